"""examples/jpeg_decode_synthetic.py (files -> decode_jpeg -> hashes, preprocess, features, against the same steps from
Pillow-decoded pixels) runs end to end on the GPU; its own assertions are the bit-for-bit comparisons."""
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


def test_jpeg_decode_example():
    imgs, status, hashes, feats = _load("jpeg_decode_synthetic").main(["--images", "12", "--model", "tiny-test", "--seed", "1"])
    assert len(imgs) == 12 and all(im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 for im in imgs)
    assert status.tolist().count(1) == 1 and status.tolist().count(0) == 11        # the progressive file went to Pillow
    assert hashes.shape == (12, 3, 1) and feats.shape[0] == 12 and torch.isfinite(feats.float()).all()
