"""Times the attention core alone through mmr_debug_attention / mmr_debug_attention_masked (development aid).
B, T, HEADS, CAUSAL, MASKED (a random key-padding mask, at least one kept key per sequence), ITERS via env; the library is
the in-tree build or the one MMR_LIB names (A/B builds)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mmr_amd import _lib

dev = torch.device("cuda:0")
B, T, H = int(os.environ.get("B", 128)), int(os.environ.get("T", 577)), int(os.environ.get("HEADS", 16))
causal, masked = int(os.environ.get("CAUSAL", 0)), int(os.environ.get("MASKED", 0))
d = H * 64
g = torch.Generator(device=dev).manual_seed(1)
qkv = (torch.randn(B * T, 3 * d, device=dev, generator=g) * 0.5).bfloat16()
o = torch.empty(B * T, d, dtype=torch.bfloat16, device=dev)
L, st = _lib.lib(), _lib.stream_ptr(dev)
if masked:
    mask = (torch.rand(B, T, device=dev, generator=g) < 0.7).int()
    mask[:, 0] = 1
    run = lambda: L.mmr_debug_attention_masked(qkv.data_ptr(), o.data_ptr(), B, T, H, mask.data_ptr(), st)
else:
    run = lambda: L.mmr_debug_attention(qkv.data_ptr(), o.data_ptr(), B, T, H, causal, st)
it = int(os.environ.get("ITERS", 20))
for _ in range(3):
    _lib.check(run())
torch.cuda.synchronize()
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
s.record()
for _ in range(it):
    run()
e.record()
torch.cuda.synchronize()
us = s.elapsed_time(e) / it * 1e3
flop = 4.0 * B * H * T * T * 64
form = "masked" if masked else ("causal" if causal else "plain")
print(f"attention B={B} T={T} heads={H} {form} lib={os.environ.get('MMR_LIB', 'in-tree')}: {us:.1f} us  {flop / us / 1e6:.0f} TFLOP/s", flush=True)
