"""Tip-Adapter-F on the device (csrc/tip_train.hip, mmr_amd.TipAdapterF) against the fp64 restatement of the step
(tip_train_helpers).  No tolerance here is a fixed number: the device may deviate from fp64 by

    8 x (what the reference's own arithmetic -- the same step in fp32 torch on the CPU -- deviates, max norm)
    + 1 fp32 ulp of the largest magnitude compared

The 8 covers the MFMA's one sequential K-long fmaf chain against the blocked sums of torch's CPU kernels; the ulp term keeps
the allowance from being zero where fp32 torch happens to be exact.  Every test prints its figures before it asserts.
"""
import functools
import importlib.util
import os

import pytest
import torch

import tip_train_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ALPHA, BETA, LR0 = 1.0, 5.5, 1e-3


def _trainer(inp, device, total_steps=20, alpha=ALPHA, beta=BETA):
    import mmr_amd as clip
    return clip.TipAdapterF(inp["cache_keys"].to(device), inp["cache_values"].to(device), inp["clip_weights"].to(device),
                            alpha, beta, lr=LR0, total_steps=total_steps)


@functools.lru_cache(maxsize=None)
def _one_step_refs(B, S, C, E, dtype, soft, alpha=ALPHA, large=False):
    """Inputs, the fp64 restatement and the fp32-torch run of one step without update; computed once per case."""
    inp = H.make_inputs(B, S, C, E, dtype=dtype, seed=B + S, soft_values=soft)
    if large:       # every feature row IS a classifier row, 100*cos = 100: its own class's (loss 0, softmax saturated) on
        # even rows, the next class's on odd rows (a loss of tens, a gradient that does not vanish)
        inp["features"] = inp["clip_weights"].t()[(inp["targets"] + torch.arange(B) % 2) % C].contiguous()
    F, y, WcT, V, W = H.as64(inp)
    loss, g, L, pred = H.restate_forward_backward(F, y, WcT, V, W, alpha, BETA)
    r32 = H.torch_train([(F, y)], WcT, V, W, alpha, BETA, LR0, 1, torch.float32, update=False)
    return inp, dict(loss=loss, grad=g, logits=L, pred=pred), r32


def _check_one_step(t, inp, r64, r32, device, what):
    loss, grad = t.loss_and_grad(inp["features"].to(device), inp["targets"].to(device))
    pred = t.pred.cpu().long()
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
    g_err, g_dev, g_all = H.max_err(grad, r64["grad"]), H.max_err(r32["grads"][0], r64["grad"]), H.allowance(r32["grads"][0], r64["grad"])
    l_err, l_dev, l_all = H.max_err(loss, r64["loss"]), H.max_err(r32["losses"][0], r64["loss"]), H.allowance(r32["losses"][0], r64["loss"])
    print(f"{what}: gradient err {g_err:.3e} (fp32 torch {g_dev:.3e}, allowance {g_all:.3e}, max|g| {float(r64['grad'].abs().max()):.3e}); "
          f"loss err {l_err:.3e} (fp32 torch {l_dev:.3e}, allowance {l_all:.3e}, loss {float(r64['loss']):.6f})")
    # pred: rows whose two best fp64 logits lie further apart than the logits' own allowance must agree
    L = r64["logits"]
    logit_all = H.allowance(r32["logits"], L)
    if L.shape[1] > 1:
        top2 = L.topk(2, dim=1).values
        sure = (top2[:, 0] - top2[:, 1]) > logit_all
    else:
        sure = torch.ones(L.shape[0], dtype=torch.bool)
    left_out = int((~sure).sum())
    print(f"{what}: logit allowance {logit_all:.3e}; {left_out} of {L.shape[0]} rows too close to call")
    assert g_err <= g_all
    assert l_err <= l_all
    assert left_out <= 0.02 * L.shape[0]
    assert torch.equal(pred[sure], r64["pred"][sure])
    assert ((pred >= 0) & (pred < L.shape[1])).all()


CASES = [(1, 1, 1, 128, torch.bfloat16, False), (33, 31, 6, 512, torch.bfloat16, True), (257, 96, 6, 512, torch.bfloat16, False),
         (257, 96, 6, 512, torch.float16, False), (257, 96, 6, 512, torch.float32, False), (64, 130, 64, 768, torch.bfloat16, False),
         (37, 96, 5, 1024, torch.bfloat16, False), (16, 16, 2, 256, torch.bfloat16, False)]


@pytest.mark.parametrize("B,S,C,E,dtype,soft", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_gradient_loss_and_pred_of_one_step(device, B, S, C, E, dtype, soft):
    inp, r64, r32 = _one_step_refs(B, S, C, E, dtype, soft)
    t = _trainer(inp, device)
    w0 = t.weight.clone()
    _check_one_step(t, inp, r64, r32, device, f"B={B} S={S} C={C} E={E} {dtype}")
    assert torch.equal(t.weight, w0) and t.steps_done == 0 and not t.exp_avg.any()       # no update
    t.check()


def test_large_logits_need_the_max_subtraction(device):
    """100*cos = 100 on every row and alpha = 10: exp(100) is not an fp32 number, so a softmax without the row maximum
    subtracted gives inf / NaN here."""
    B, S, C, E = 33, 31, 6, 512
    inp, r64, r32 = _one_step_refs(B, S, C, E, torch.bfloat16, False, alpha=10.0, large=True)
    assert float(r64["logits"].max()) > 99.0 and float(r64["loss"]) > 1.0 and float(r64["grad"].abs().max()) > 1e-3
    assert not torch.isfinite(torch.exp(r64["logits"].float())).all()            # what the subtraction is for
    _check_one_step(_trainer(inp, device, alpha=10.0), inp, r64, r32, device, "large logits")


@functools.lru_cache(maxsize=None)
def _trajectory(bad_labels=False, steps=20):
    B, S, C, E = (33, 96, 6, 512) if bad_labels else (37, 96, 6, 512)
    inp = H.make_inputs(B, S, C, E, seed=11)
    F, y, WcT, V, W = H.as64(inp)
    g = torch.Generator().manual_seed(12)
    batches = []
    for _ in range(steps):
        rows = torch.randint(0, B, (B,), generator=g)
        yb = y[rows].clone()
        if bad_labels:
            yb[5], yb[20] = -1, C
        batches.append((inp["features"][rows].contiguous(), yb))
    b64 = [(f.double(), yb) for f, yb in batches]
    r64 = H.restate_train(b64, WcT, V, W, ALPHA, BETA, LR0, steps, **H.ADAMW)
    r32 = H.torch_train(b64, WcT, V, W, ALPHA, BETA, LR0, steps, torch.float32)
    return inp, batches, r64, r32


def _compare_state(t, losses, r64, r32, what):
    for name, dev in (("weight", t.weight), ("exp_avg", t.exp_avg), ("exp_avg_sq", t.exp_avg_sq), ("losses", losses)):
        err, ref_dev, allow = H.max_err(dev, r64[name]), H.max_err(r32[name], r64[name]), H.allowance(r32[name], r64[name])
        print(f"{what} {name}: err {err:.3e} (fp32 torch {ref_dev:.3e}, allowance {allow:.3e}, max magnitude "
              f"{float(r64[name].abs().max()):.3e})")
    for name, dev in (("weight", t.weight), ("exp_avg", t.exp_avg), ("exp_avg_sq", t.exp_avg_sq), ("losses", losses)):
        assert H.max_err(dev, r64[name]) <= H.allowance(r32[name], r64[name]), name


def test_trajectory_of_20_steps_under_the_cosine_schedule(device):
    inp, batches, r64, r32 = _trajectory()
    t = _trainer(inp, device, total_steps=20)
    losses = torch.stack([t.step(f.to(device), y.to(device)) for f, y in batches])
    assert t.steps_done == 20
    _compare_state(t, losses, r64, r32, "20 steps")
    t.check()
    with pytest.raises(RuntimeError):
        t.step(batches[0][0].to(device), batches[0][1].to(device))        # the schedule is used up


def _ulps(x):
    """fp32 ulp at every element of an fp64 tensor."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


def test_adamw_alone_from_the_devices_own_gradient(device):
    """W, m, v before a step and the gradient the device itself used -> the update in fp64.  Fewer than 16 roundings of
    half an ulp lie between the inputs and the update's size (2^-20 of it), the final store adds half an ulp of W; m and
    v are two or three roundings each.  Steps 1, 2 and 20 have different bias corrections."""
    inp, batches, _, _ = _trajectory()
    t = _trainer(inp, device, total_steps=20)
    grad = torch.empty_like(t.weight)
    for i, (f, y) in enumerate(batches):
        step = i + 1
        if step not in (1, 2, 20):
            t.step(f.to(device), y.to(device))
            continue
        w0, m0, v0 = t.weight.double().cpu(), t.exp_avg.double().cpu(), t.exp_avg_sq.double().cpu()
        t.step(f.to(device), y.to(device), grad_out=grad)
        w1, m1, v1 = H.restate_adamw(w0, m0, v0, grad.double().cpu(), H.cosine_lr(LR0, i, 20), step, **H.ADAMW)
        ew, em, ev = (t.weight.double().cpu() - w1).abs(), (t.exp_avg.double().cpu() - m1).abs(), (t.exp_avg_sq.double().cpu() - v1).abs()
        bound_w = _ulps(w1) + 2.0 ** -20 * (w1 - w0).abs()
        print(f"step {step}: W err / bound {float((ew / bound_w).max()):.3f}, m err {float((em / _ulps(m1)).max()):.3f} ulp, "
              f"v err {float((ev / _ulps(v1)).max()):.3f} ulp; max|dW| {float((w1 - w0).abs().max()):.3e}")
        assert (ew <= bound_w).all()
        assert (em <= 2 * _ulps(m1)).all()
        assert (ev <= 2 * _ulps(v1)).all()
        assert float((w1 - w0).abs().max()) > 0


def test_two_trainers_agree_bit_for_bit_and_fit_equals_steps(device):
    inp, batches, _, _ = _trajectory()
    a, b = _trainer(inp, device), _trainer(inp, device)
    la = torch.stack([a.step(f.to(device), y.to(device)) for f, y in batches[:5]])
    lb = torch.stack([b.step(f.to(device), y.to(device)) for f, y in batches[:5]])
    for x, z in ((a.weight, b.weight), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq), (la, lb)):
        assert torch.equal(x, z)
    assert float((a.weight - inp["cache_keys"].t().to(device)).abs().max()) > 0

    # fit: 100 rows in batches of 32 (the last holds 4), two epochs, against the same eight step calls
    big = H.make_inputs(100, 96, 6, 512, seed=13)
    f, y = big["features"].to(device), big["targets"].to(device)
    c, d = _trainer(big, device), _trainer(big, device)
    lc = c.fit(f, y, 32, 2)
    ld = torch.stack([d.step(f[lo:lo + 32], y[lo:lo + 32]) for _ in range(2) for lo in range(0, 100, 32)])
    assert lc.shape == (8,) and c.steps_done == d.steps_done == 8
    for x, z in ((c.weight, d.weight), (c.exp_avg, d.exp_avg), (c.exp_avg_sq, d.exp_avg_sq), (lc, ld)):
        assert torch.equal(x, z)
    # a generator shuffles: same seed, same bits; and not the unshuffled run's
    e, g = _trainer(big, device), _trainer(big, device)
    le = e.fit(f, y, 32, 2, generator=torch.Generator().manual_seed(5))
    lg = g.fit(f, y, 32, 2, generator=torch.Generator().manual_seed(5))
    assert torch.equal(le, lg) and torch.equal(e.weight, g.weight) and not torch.equal(le, lc)
    with pytest.raises(RuntimeError):
        e.fit(f, y, 32, 4)                   # 16 more steps after 8 of 20


def _raw(device, inp, B=None, pad=0, ws_fill=0, update=True, step=1):
    """One call through the C ABI with ctypes.  Every output buffer holds `pad` extra elements set to a sentinel."""
    from mmr_amd import _lib
    L = _lib.lib()
    f, y = inp["features"].to(device), inp["targets"].to(device)
    B = f.shape[0] if B is None else B
    wct = inp["clip_weights"].t().contiguous().to(device)
    V = inp["cache_values"].to(device)
    S, E = inp["cache_keys"].shape[1], inp["cache_keys"].shape[0]
    C = V.shape[1]

    def padded(x, sentinel):
        buf = torch.full((x.numel() + pad,), sentinel, dtype=x.dtype, device=device)
        buf[:x.numel()] = x.reshape(-1)
        return buf
    W = padded(inp["cache_keys"].t().contiguous().to(device), 12345.0)
    m, v = padded(torch.zeros(S * E, device=device), 12345.0), padded(torch.zeros(S * E, device=device), 12345.0)
    grad = padded(torch.full((S * E,), -3.0, device=device), 12345.0)
    loss = padded(torch.full((1,), -3.0, device=device), 12345.0)
    pred = padded(torch.full((max(B, 1),), -3, dtype=torch.int32, device=device), -77)
    status = torch.zeros(2, dtype=torch.int32, device=device)
    status[1] = -77
    need = L.mmr_tip_adapter_f_workspace_bytes(max(B, 1), E, C, S)
    ws = torch.full((need + 16,), ws_fill, dtype=torch.uint8, device=device)
    rc = L.mmr_tip_adapter_f_step(f.data_ptr(), y.data_ptr(), _lib.dtype_code(f.dtype), B, E, C, S, wct.data_ptr(), V.data_ptr(),
                                  W.data_ptr(), m.data_ptr() if update else 0, v.data_ptr() if update else 0, ALPHA, BETA,
                                  LR0, 0.9, 0.999, 1e-4, 0.01, step, loss.data_ptr(), pred.data_ptr(), grad.data_ptr(),
                                  status.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr(device))
    torch.cuda.synchronize()
    return rc, dict(W=W, m=m, v=v, grad=grad, loss=loss, pred=pred, status=status, ws=ws, need=need)


def test_workspace_contents_do_not_matter(device):
    inp = H.make_inputs(33, 31, 6, 256, seed=21)
    rc0, a = _raw(device, inp, ws_fill=0)
    rc1, b = _raw(device, inp, ws_fill=0xFF)
    assert rc0 == 0 and rc1 == 0
    for k in ("W", "m", "v", "grad", "loss", "pred", "status"):
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a["loss"]).all() and float(a["grad"].abs().max()) > 0


@pytest.mark.parametrize("B,S,C,E", [(33, 31, 6, 128), (1, 1, 1, 128), (17, 130, 64, 256)])
def test_nothing_is_written_out_of_bounds(device, B, S, C, E):
    inp = H.make_inputs(B, S, C, E, seed=22)
    rc, o = _raw(device, inp, pad=1)
    assert rc == 0
    for k in ("W", "m", "v", "grad", "loss"):
        assert float(o[k][-1]) == 12345.0, k
        assert torch.isfinite(o[k][:-1]).all() and not (o[k][:-1] == -3.0).any(), k          # and all of it was written
    assert int(o["pred"][-1]) == -77 and ((o["pred"][:-1] >= 0) & (o["pred"][:-1] < C)).all()
    assert o["status"].tolist() == [0, -77]
    assert (o["ws"][o["need"]:] == 0).all()                                                  # the workspace's end holds
    # no update: weight and state untouched, loss / pred / grad written
    rc, n = _raw(device, inp, pad=1, update=False)
    assert rc == 0 and torch.equal(n["W"][:-1], inp["cache_keys"].t().reshape(-1).to(device)) and not n["m"][:-1].any()
    assert torch.equal(n["grad"], o["grad"]) and torch.equal(n["loss"], o["loss"]) and torch.equal(n["pred"], o["pred"])


def test_an_empty_batch_returns_ok_and_writes_nothing(device):
    inp = H.make_inputs(4, 7, 3, 128, seed=23)
    rc, o = _raw(device, inp, B=0, pad=1)
    assert rc == 0
    assert torch.equal(o["W"][:-1], inp["cache_keys"].t().reshape(-1).to(device))
    assert not o["m"][:-1].any() and not o["v"][:-1].any()
    assert (o["grad"][:-1] == -3.0).all() and float(o["loss"][0]) == -3.0 and int(o["pred"][0]) == -3
    assert o["status"].tolist() == [0, -77] and not o["ws"].any()


def test_labels_outside_the_classes_take_no_part_and_are_reported(device):
    inp, batches, r64, r32 = _trajectory(bad_labels=True, steps=3)
    t = _trainer(inp, device, total_steps=3)
    losses = torch.stack([t.step(f.to(device), y.to(device)) for f, y in batches])
    assert int(t._status.item()) == 1
    with pytest.raises(ValueError):
        t.check()
    assert ((t.pred >= 0) & (t.pred < 6)).all()                       # pred is written for those rows too
    _compare_state(t, losses, r64, r32, "labels -1 and C")
    # all labels valid: the word stays 0
    ok_inp, ok_batches, _, _ = _trajectory()
    ok = _trainer(ok_inp, device)
    ok.step(ok_batches[0][0].to(device), ok_batches[0][1].to(device))
    assert int(ok._status.item()) == 0
    ok.check()


def test_logits_are_tip_adapter_logits_with_the_trained_keys(device, tmp_path):
    import mmr_amd as clip
    inp, batches, _, _ = _trajectory()
    t = _trainer(inp, device)
    for f, y in batches[:3]:
        t.step(f.to(device), y.to(device))
    f = inp["features"].to(device)
    want = clip.tip_adapter_logits(f, inp["clip_weights"].to(device), t.cache_keys(), inp["cache_values"].to(device), ALPHA, BETA)
    assert torch.equal(t.logits(f), want)
    assert t.cache_keys().shape == (512, 96) and torch.equal(t.cache_keys().t(), t.weight)
    t.save(tmp_path, 16)
    assert torch.equal(clip.TipAdapterF.load_weight(tmp_path, 16, device=device), t.weight)


def test_the_examples_recipe_lowers_the_loss(device):
    """C = 6, 16 shots, E = 128, 256 rows in batches of 64, 20 epochs, lr 1e-3, alpha 1, beta 5.5.  With the reference's
    torch code on the CPU the last epoch's mean loss is 12-14 % below the first's for seeds 0-5.  Accuracy moves by under
    a point either way, so it is printed and not asserted."""
    spec = importlib.util.spec_from_file_location("tip_adapter_f_synthetic", os.path.join(ROOT, "examples", "tip_adapter_f_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for seed in (0, 1):
        epoch_losses, acc_before, acc_after = mod.main(["--seed", str(seed)])
        print(f"seed {seed}: mean loss {epoch_losses[0]:.4f} -> {epoch_losses[-1]:.4f}; held-out accuracy {acc_before:.4f} -> {acc_after:.4f}")
        assert len(epoch_losses) == 20
        assert epoch_losses[-1] < epoch_losses[0]
