"""examples/tip_adapter_augment_synthetic.py (augmented cache build, then Tip-Adapter-F steps on freshly augmented
features) runs end to end on the GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tip_adapter_augment_example():
    keys, values, losses = _load("tip_adapter_augment_synthetic").main(["--seed", "1", "--model", "tiny-test"])
    assert keys.shape[1] == 12 and values.shape == (12, 3)
    assert torch.allclose(keys.float().norm(dim=0).cpu(), torch.ones(12), atol=1e-3)
    assert len(losses) == 8 and np.isfinite(losses).all()
