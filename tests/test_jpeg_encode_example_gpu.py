"""examples/jpeg_encode_synthetic.py (synthetic RGBA / RGB / greyscale pixels -> encode_jpeg -> decode_jpeg, against Pillow's
save and open) runs end to end on the GPU; its own assertions are the byte-for-byte comparisons."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_jpeg_encode_example(tmp_path):
    ours, theirs, decoded = _load("jpeg_encode_synthetic").main(["--images", "9", "--seed", "1", "--out", str(tmp_path)])
    assert len(ours) == 9 and ours == theirs and all(f[:2] == b"\xff\xd8" and f[-2:] == b"\xff\xd9" for f in ours)
    assert all(d.dtype == torch.uint8 and d.dim() == 3 and d.shape[2] == 3 for d in decoded)
    assert sorted(os.listdir(tmp_path)) == [f"image_{i:03d}.jpg" for i in range(9)]
