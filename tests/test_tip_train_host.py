"""Tip-Adapter-F without a GPU: the closed-form restatement of the step (tip_train_helpers) reproduces torch autograd +
torch.optim.AdamW(eps=1e-4) + CosineAnnealingLR in fp64, the C ABI declares the two entry points, and TipAdapterF checks
its arguments before any device call."""
import os

import pytest
import torch

import tip_train_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("B,S,C,E", [(37, 96, 6, 512), (5, 3, 2, 128)])
def test_restatement_is_torch_autograd_adamw_cosine_in_fp64(B, S, C, E):
    steps, lr0, alpha, beta = 20, 1e-3, 1.0, 5.5
    inp = H.make_inputs(B, S, C, E, seed=3)
    F, y, WcT, V, W = H.as64(inp)
    g = torch.Generator().manual_seed(4)
    batches = []
    for _ in range(steps):                               # a new batch every step: rows drawn from the recipe's
        rows = torch.randint(0, B, (B,), generator=g)
        batches.append((F[rows], y[rows]))
    ours = H.restate_train(batches, WcT, V, W, alpha, beta, lr0, steps, **H.ADAMW)
    ref = H.torch_train(batches, WcT, V, W, alpha, beta, lr0, steps, torch.float64)
    dw = float((ours["weight"] - ref["weight"]).abs().max())
    dlr = max(abs(a - b) / b for a, b in zip(ours["lrs"], ref["lrs"]))
    dl = float((ours["losses"] - ref["losses"]).abs().max())
    print(f"weights {dw:.2e} abs, learning rates {dlr:.2e} rel, losses {dl:.2e} abs")
    assert dw <= 1e-12
    assert dlr <= 1e-12
    assert dl <= 1e-12
    assert float((ours["exp_avg"] - ref["exp_avg"]).abs().max()) <= 1e-12
    assert float((ours["exp_avg_sq"] - ref["exp_avg_sq"]).abs().max()) <= 1e-12
    assert float((ours["weight"] - W).abs().max()) > 1e-4            # it did train (eps = 1e-4 damps the small gradients)


def test_restatement_bad_labels_take_no_part():
    B, S, C, E = 9, 7, 3, 128
    F, y, WcT, V, W = H.as64(H.make_inputs(B, S, C, E, seed=5))
    y = y.clone()
    y[2], y[6] = -1, C
    loss, g, L, pred = H.restate_forward_backward(F, y, WcT, V, W, 1.0, 5.5)
    keep = torch.tensor([i for i in range(B) if i not in (2, 6)])
    loss_k, g_k, L_k, pred_k = H.restate_forward_backward(F[keep], y[keep], WcT, V, W, 1.0, 5.5)
    # the valid rows alone, with the divisor put back to B
    assert abs(float(loss) - float(loss_k) * len(keep) / B) <= 1e-14
    assert float((g - g_k * len(keep) / B).abs().max()) <= 1e-16
    assert torch.equal(pred[keep], pred_k) and pred.shape == (B,)     # pred is written for every row
    ref = H.torch_train([(F, y)], WcT, V, W, 1.0, 5.5, 1e-3, 1, torch.float64, update=False)
    assert abs(float(loss) - float(ref["losses"][0])) <= 1e-13
    assert float((g - ref["grads"][0]).abs().max()) <= 1e-15


def test_restatement_argmax_takes_the_lowest_class_on_a_tie():
    F = torch.zeros(2, 128, dtype=torch.float64)
    WcT = torch.zeros(3, 128, dtype=torch.float64)
    V = torch.tensor([[0.0, 1.0, 1.0]], dtype=torch.float64)
    W = torch.zeros(1, 128, dtype=torch.float64)
    _, _, L, pred = H.restate_forward_backward(F, torch.tensor([0, 1]), WcT, V, W, 1.0, 1.0)
    assert L[0, 1] == L[0, 2] > L[0, 0] and pred.tolist() == [1, 1]


def test_header_declares_the_step_and_its_workspace():
    import ctypes

    from mmr_amd import _header
    fns = _header.load().functions
    p, i, i64, f, d, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
    res, args, names = fns["mmr_tip_adapter_f_workspace_bytes"]
    assert res is sz and args == [i64, i, i, i] and names == ["B", "E", "C", "S"]
    res, args, names = fns["mmr_tip_adapter_f_step"]
    assert res is i
    assert names == ["features", "targets", "dtype", "B", "E", "C", "S", "clip_weights_t", "cache_values", "weight", "exp_avg",
                     "exp_avg_sq", "alpha", "beta", "lr", "beta1", "beta2", "eps", "weight_decay", "step", "loss", "pred",
                     "grad_out", "status", "workspace", "workspace_bytes", "stream"]
    assert args == [p, p, i, i64, i, i, i, p, p, p, p, p, f, f, d, d, d, d, d, i64, p, p, p, p, p, sz, p]


def test_names_are_exported():
    import mmr_amd
    assert "TipAdapterF" in mmr_amd.__all__ and "cosine_lr" in mmr_amd.__all__
    assert mmr_amd.TipAdapterF is mmr_amd.tip_adapter.TipAdapterF
    assert mmr_amd.cosine_lr(1e-3, 0, 20) == 1e-3
    assert mmr_amd.cosine_lr(1e-3, 10, 20) == pytest.approx(5e-4, rel=1e-15)
    assert [mmr_amd.cosine_lr(1e-3, t, 20) for t in range(20)] == [H.cosine_lr(1e-3, t, 20) for t in range(20)]


def _cpu_args(E=128, S=12, C=3, dtype=torch.bfloat16):
    return torch.zeros(E, S), torch.zeros(S, C), torch.zeros(E, C, dtype=dtype)


def test_constructor_refuses_bad_arguments_before_any_device_call():
    from mmr_amd import TipAdapterF
    k, v, w = _cpu_args()
    kw = dict(alpha=1.0, beta=5.5, total_steps=4)
    with pytest.raises(ValueError):
        TipAdapterF(k[:, :5], v, w, **kw)                       # S of the keys and of the values differ
    with pytest.raises(ValueError):
        TipAdapterF(k, v, w[:, :2], **kw)                       # C differs
    with pytest.raises(ValueError):
        TipAdapterF(k[:100], v, w[:100], **kw)                  # E = 100 is no width the kernels take
    with pytest.raises(ValueError):
        TipAdapterF(k, torch.zeros(12, 65), torch.zeros(128, 65, dtype=torch.bfloat16), **kw)     # C > 64
    with pytest.raises(ValueError):
        TipAdapterF(k[0], v, w, **kw)                           # not 2-D
    with pytest.raises(ValueError):
        TipAdapterF(k, v, w.double(), **kw)                     # a classifier dtype the kernels do not read
    with pytest.raises(ValueError):
        TipAdapterF(k, v.long(), w, **kw)                       # integer values
    with pytest.raises(ValueError):
        TipAdapterF(k, v, w, alpha=1.0, beta=5.5)               # the schedule needs its length
    with pytest.raises(RuntimeError, match="GPU"):
        TipAdapterF(k, v, w, **kw)                              # all well but on the CPU


def test_batches_are_checked_before_any_device_call():
    """_check_batch is what step, fit and loss_and_grad run first; it needs no device."""
    from mmr_amd import TipAdapterF
    t = TipAdapterF.__new__(TipAdapterF)
    t.E, t.S, t.C = 128, 12, 3
    t._wct = torch.zeros(3, 128, dtype=torch.bfloat16)
    f, y = torch.zeros(5, 128, dtype=torch.bfloat16), torch.zeros(5, dtype=torch.int64)
    for bad_f, bad_y in ((f[:, :64], y), (f[0], y), (f, y[:4]), (f, y[:, None]), (f.float(), y), (f.half(), y), (f, y.int()),
                         (f, y.float())):
        with pytest.raises(ValueError):
            t._check_batch(bad_f, bad_y)
        for call in (t.step, t.loss_and_grad, lambda a, b: t.fit(a, b, 2, 1)):
            with pytest.raises(ValueError):
                call(bad_f, bad_y)
    for call in (t.step, t.loss_and_grad, lambda a, b: t.fit(a, b, 2, 1)):
        with pytest.raises(RuntimeError, match="GPU"):
            call(f, y)


def test_weight_file_round_trip(tmp_path):
    from mmr_amd import TipAdapterF
    w = torch.randn(12, 128, generator=torch.Generator().manual_seed(1))
    path = TipAdapterF.save_weight(w, tmp_path, 16)
    assert os.path.basename(path) == "best_F_16shots.pt"                 # main_custom.py:212
    assert torch.equal(TipAdapterF.load_weight(tmp_path, 16), w)
    t = TipAdapterF.__new__(TipAdapterF)
    t.weight = w * 2
    assert t.save(tmp_path, 4) == os.path.join(str(tmp_path), "best_F_4shots.pt")
    assert torch.equal(TipAdapterF.load_weight(tmp_path, 4), w * 2)
    # the reference stores the nn.Parameter itself, in the model's fp16
    torch.save(torch.nn.Parameter(w.half()), os.path.join(str(tmp_path), "best_F_1shots.pt"))
    back = TipAdapterF.load_weight(tmp_path, 1)
    assert back.dtype == torch.float16 and not back.requires_grad and torch.equal(back, w.half())
    torch.save({"weight": w}, os.path.join(str(tmp_path), "best_F_2shots.pt"))
    with pytest.raises(ValueError):
        TipAdapterF.load_weight(tmp_path, 2)


def test_ulp_and_allowance_helpers():
    assert H.ulp32(1.0) == 2.0 ** -23 and H.ulp32(1.5) == 2.0 ** -23 and H.ulp32(0.75) == 2.0 ** -24
    assert H.ulp32(0.0) == 2.0 ** -149 and H.ulp32(100.0) == 2.0 ** -17
    a = H.allowance(torch.tensor([1.0, 2.0 + 2.0 ** -20], dtype=torch.float64), torch.tensor([1.0, 2.0], dtype=torch.float64))
    assert a == 8 * 2.0 ** -20 + 2.0 ** -22
