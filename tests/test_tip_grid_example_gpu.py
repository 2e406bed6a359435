"""examples/tip_adapter_search_hp_synthetic.py (the search that ends the reference's run_tip_adapter and
run_tip_adapter_F) runs end to end on the GPU, with the cache as built and with trained keys."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("extra", [[], ["--train"]], ids=["cache", "trained"])
def test_tip_adapter_search_hp_example(extra):
    mod = _load("tip_adapter_search_hp_synthetic")
    beta, alpha, score, per_class = mod.main(["--seed", "3", "--dim", "256"] + extra)
    betas, alphas = (
        [i * 7 / 10 + 0.01 for i in range(10)], [i * 3 / 6 + 0.01 for i in range(6)])
    assert beta in betas and alpha in alphas
    assert 0.5 < score <= 1.0                            # far above chance: the classes are separable by construction
    assert len(per_class) == 6 and all(0.0 <= f <= 1.0 for f in per_class)
