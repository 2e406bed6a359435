"""examples/tip_adapter_f_synthetic.py (the flow of the reference's run_tip_adapter_F) runs end to end on the GPU."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tip_adapter_f_example():
    epoch_losses, acc_before, acc_after = _load("tip_adapter_f_synthetic").main(["--seed", "3", "--dim", "256"])
    assert len(epoch_losses) == 20 and np.isfinite(epoch_losses).all()
    assert epoch_losses[-1] < epoch_losses[0]
    assert 0.0 <= acc_before <= 1.0 and 0.0 <= acc_after <= 1.0
    assert acc_after > 1.0 / 6 + 0.2                     # far above chance: the classes are separable by construction
