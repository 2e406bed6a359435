"""Tip-Adapter-F: fine-tune the cache keys on the device (reference code/main_custom.py:148-247, `run_tip_adapter_F`).

The reference makes the cache keys learnable as ``adapter = nn.Linear(E, S)`` with ``adapter.weight = cache_keys.t()``
and trains that one matrix with ``AdamW(eps=1e-4)`` under ``CosineAnnealingLR`` for 20 epochs; the encoder is frozen.
One step is therefore closed-form arithmetic -- two small matrix products, an exponential, a softmax and an element-wise
optimizer -- and runs here as two HIP launches (csrc/tip_train.hip, ``mmr_tip_adapter_f_step``) with no autograd, no
host synchronisation and no device-to-host copy.  The master weight stays fp32 whatever the features' dtype.

The (beta, alpha) grid search that ends both of the reference's drivers (``search_hp``, code/utils.py:159-206) is the
second half of this module: ``tip_adapter_grid`` scores every grid point in three launches (csrc/tip_grid.hip,
``mmr_tip_adapter_grid``) -- the reference's per-class threshold F1, exact in fp64, and the confusion counts behind
``cls_f1`` and ``cls_acc`` -- and ``search_hp`` / ``TipAdapterF.search_hp`` pick the pair by the reference's rule.
"""
import math
import os
from typing import Optional, Tuple

import torch

from . import _lib
from .search import _NATIVE_DTYPES, tip_adapter_logits

_WIDTHS = (128, 256, 512, 768, 1024)
_C_MAX, _S_MAX = 64, 16384


def cosine_lr(lr0: float, t: int, total_steps: int) -> float:
    """``CosineAnnealingLR(T_max=total_steps, eta_min=0)`` in closed form: the rate of step ``t`` (from 0), in fp64."""
    return lr0 * (1.0 + math.cos(math.pi * t / total_steps)) / 2.0


def _weight_path(cache_dir, shots) -> str:
    return os.path.join(str(cache_dir), "best_F_" + str(shots) + "shots.pt")


class TipAdapterF:
    """The learnable cache of Tip-Adapter-F and its optimizer state.

        t = TipAdapterF(cache_keys[E,S], cache_values[S,C], clip_weights[E,C], alpha, beta, lr=1e-3, total_steps=T)
        loss = t.step(features[B,E], targets[B])        # 0-d fp32 device tensor; nothing is read back
        losses = t.fit(features[N,E], targets[N], batch_size, epochs)
        tip_logits = t.logits(test_features)            # tip_adapter_logits with the trained keys

    ``weight`` [S,E] (= ``adapter.weight``), ``exp_avg``, ``exp_avg_sq`` are fp32 device tensors; ``steps_done`` counts
    the updates.  Features and ``clip_weights`` share one dtype (bf16, fp16 or fp32) and are consumed as they are.
    Labels outside [0,C) take no part in a step and are reported by ``check()``.
    """

    def __init__(self, cache_keys: torch.Tensor, cache_values: torch.Tensor, clip_weights: torch.Tensor, alpha: float,
                 beta: float, lr: float = 1e-3, total_steps: Optional[int] = None, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-4, weight_decay: float = 0.01):
        for name, x in (("cache_keys", cache_keys), ("cache_values", cache_values), ("clip_weights", clip_weights)):
            if not isinstance(x, torch.Tensor) or x.dim() != 2 or not x.is_floating_point():
                raise ValueError(f"{name} must be a 2-D floating-point tensor")
        E, S = cache_keys.shape
        C = cache_values.shape[1]
        if cache_values.shape[0] != S or tuple(clip_weights.shape) != (E, C):
            raise ValueError(f"shape mismatch: cache_keys {tuple(cache_keys.shape)} [E,S], cache_values "
                             f"{tuple(cache_values.shape)} [S,C], clip_weights {tuple(clip_weights.shape)} [E,C]")
        if E not in _WIDTHS or not 1 <= C <= _C_MAX or not 1 <= S <= _S_MAX:
            raise ValueError(f"E={E} must be one of {_WIDTHS}, 1 <= C={C} <= {_C_MAX}, 1 <= S={S} <= {_S_MAX}")
        if clip_weights.dtype not in _NATIVE_DTYPES:
            raise ValueError(f"clip_weights must be float32, bfloat16 or float16, got {clip_weights.dtype}")
        if total_steps is None or int(total_steps) < 1:
            raise ValueError("total_steps (the cosine schedule's length) must be >= 1")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or eps < 0.0 or lr < 0.0:
            raise ValueError(f"bad optimizer settings: lr={lr} betas={betas} eps={eps}")
        for name, x in (("cache_keys", cache_keys), ("cache_values", cache_values), ("clip_weights", clip_weights)):
            if not x.is_cuda:
                raise RuntimeError(f"{name} must live on the GPU (there is no CPU path)")
        dev = cache_keys.device
        self.E, self.S, self.C = E, S, C
        self.alpha, self.beta = float(alpha), float(beta)
        self.lr, self.total_steps = float(lr), int(total_steps)
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.clip_weights = clip_weights.to(dev)
        self.cache_values = cache_values.to(dev, torch.float32).contiguous()
        self._wct = self.clip_weights.t().contiguous()                              # [C,E], the features' dtype
        self.weight = cache_keys.t().to(torch.float32).contiguous().clone()        # [S,E] fp32 master copy
        self.exp_avg = torch.zeros_like(self.weight)
        self.exp_avg_sq = torch.zeros_like(self.weight)
        self.steps_done = 0
        self.pred = None                                                           # int32 [B]: the last call's arg-max
        self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ws = None

    # ------------------------------------------------------------------ checks, before anything touches the device
    def _check_batch(self, features, targets):
        if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[1] != self.E:
            raise ValueError(f"features must be [B,{self.E}], got {tuple(getattr(features, 'shape', ()))}")
        if not isinstance(targets, torch.Tensor) or targets.dim() != 1 or targets.shape[0] != features.shape[0]:
            raise ValueError(f"targets must be [B] = [{features.shape[0]}], got {tuple(getattr(targets, 'shape', ()))}")
        if features.dtype != self._wct.dtype:
            raise ValueError(f"features are {features.dtype} but clip_weights are {self._wct.dtype}: one dtype for both")
        if targets.dtype != torch.int64:
            raise ValueError(f"targets must be int64, got {targets.dtype}")
        if not features.is_cuda or not targets.is_cuda:
            raise RuntimeError("features and targets must live on the GPU (there is no CPU path)")

    def _workspace(self, B: int):
        need = _lib.lib().mmr_tip_adapter_f_workspace_bytes(B, self.E, self.C, self.S)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.weight.device)
        return self._ws

    def _call(self, features, targets, loss_ptr: int, update: bool, lr: float, grad_out):
        f, y = features.contiguous(), targets.contiguous()
        B = f.shape[0]
        if B == 0:
            raise ValueError("an empty batch has no mean loss")
        if grad_out is not None and (grad_out.shape != self.weight.shape or grad_out.dtype != torch.float32
                                     or not grad_out.is_cuda or not grad_out.is_contiguous()):
            raise ValueError(f"grad_out must be a contiguous fp32 device tensor {tuple(self.weight.shape)}")
        ws = self._workspace(B)
        if self.pred is None or self.pred.shape[0] != B:
            self.pred = torch.empty(B, dtype=torch.int32, device=f.device)
        _lib.check(_lib.lib().mmr_tip_adapter_f_step(
            f.data_ptr(), y.data_ptr(), _lib.dtype_code(f.dtype), B, self.E, self.C, self.S, self._wct.data_ptr(),
            self.cache_values.data_ptr(), self.weight.data_ptr(), self.exp_avg.data_ptr() if update else 0,
            self.exp_avg_sq.data_ptr() if update else 0, self.alpha, self.beta, lr, self.betas[0], self.betas[1], self.eps,
            self.weight_decay, self.steps_done + 1, loss_ptr, self.pred.data_ptr(), _lib.ptr(grad_out),
            self._status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(f.device)))

    def _train(self, features, targets, loss_ptr: int, grad_out=None):
        if self.steps_done >= self.total_steps:
            raise RuntimeError(f"the schedule has {self.total_steps} steps and all of them are taken")
        self._call(features, targets, loss_ptr, True, cosine_lr(self.lr, self.steps_done, self.total_steps), grad_out)
        self.steps_done += 1

    # ------------------------------------------------------------------ training
    def step(self, features: torch.Tensor, targets: torch.Tensor, grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One AdamW step at the schedule's current rate; returns the batch's mean loss (before the update) as a 0-d
        device tensor.  ``grad_out`` [S,E] fp32, if given, receives the gradient the update used."""
        self._check_batch(features, targets)
        loss = torch.empty((), dtype=torch.float32, device=features.device)
        self._train(features, targets, loss.data_ptr(), grad_out)
        return loss

    def fit(self, features: torch.Tensor, targets: torch.Tensor, batch_size: int, epochs: int,
            generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """``epochs`` passes over ``features`` [N,E] in batches of ``batch_size`` (the last may be short); every step is
        enqueued and the losses come back as one [steps] device tensor.  A ``generator`` shuffles the rows anew each
        epoch (``torch.randperm`` on the CPU); without one the rows are taken in order."""
        self._check_batch(features, targets)
        N = features.shape[0]
        if N == 0 or int(batch_size) < 1 or int(epochs) < 0:
            raise ValueError(f"fit needs rows, batch_size >= 1 and epochs >= 0 (N={N} batch_size={batch_size} epochs={epochs})")
        per_epoch = (N + batch_size - 1) // batch_size
        if self.steps_done + per_epoch * epochs > self.total_steps:
            raise RuntimeError(f"{per_epoch * epochs} more steps after {self.steps_done} exceed total_steps={self.total_steps}")
        f, y = features.contiguous(), targets.contiguous()
        losses = torch.empty(per_epoch * epochs, dtype=torch.float32, device=f.device)
        i = 0
        for _ in range(epochs):
            perm = None if generator is None else torch.randperm(N, generator=generator).to(f.device)
            for lo in range(0, N, batch_size):
                if perm is None:
                    fb, yb = f[lo:lo + batch_size], y[lo:lo + batch_size]
                else:
                    rows = perm[lo:lo + batch_size]
                    fb, yb = f[rows], y[rows]
                self._train(fb, yb, losses.data_ptr() + 4 * i)
                i += 1
        return losses

    def loss_and_grad(self, features: torch.Tensor, targets: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The mean loss and the gradient of ``weight`` [S,E] for one batch; nothing is updated."""
        self._check_batch(features, targets)
        loss = torch.empty((), dtype=torch.float32, device=features.device)
        grad = torch.empty_like(self.weight)
        self._call(features, targets, loss.data_ptr(), False, 0.0, grad)
        return loss, grad

    def check(self) -> None:
        """Reads the status word (one device-to-host copy); raises if any batch so far held a label outside [0,C)."""
        if int(self._status.item()) & 1:
            raise ValueError(f"a target outside [0, {self.C}) was met; such rows took no part in their steps")

    # ------------------------------------------------------------------ scoring with the trained keys
    def cache_keys(self) -> torch.Tensor:
        """``weight.t()`` [E,S]: what ``tip_adapter_logits`` takes."""
        return self.weight.t()

    def logits(self, features: torch.Tensor, return_clip_logits: bool = False):
        return tip_adapter_logits(features, self.clip_weights, self.cache_keys(), self.cache_values, self.alpha, self.beta,
                                  return_clip_logits=return_clip_logits)

    # ------------------------------------------------------------------ the reference's file (main_custom.py:212,214)
    def search_hp(self, cfg, features: torch.Tensor, labels: torch.Tensor, classes=None, criterion: str = "threshold_f1"):
        """The reference's ``search_hp(..., adapter=adapter)`` with the trained keys and this cache's values."""
        return search_hp(cfg, None, self.cache_values, features, labels, self.clip_weights, adapter=self, classes=classes,
                         criterion=criterion)

    @staticmethod
    def save_weight(weight: torch.Tensor, cache_dir, shots) -> str:
        """``best_F_{shots}shots.pt`` = ``adapter.weight`` [S,E], as a plain CPU tensor."""
        path = _weight_path(cache_dir, shots)
        torch.save(weight.detach().cpu().contiguous(), path)
        return path

    def save(self, cache_dir, shots) -> str:
        return self.save_weight(self.weight, cache_dir, shots)

    @staticmethod
    def load_weight(cache_dir, shots, device=None) -> torch.Tensor:
        """``adapter.weight`` [S,E] from ``best_F_{shots}shots.pt`` (ours or the reference's, which holds an fp16
        ``nn.Parameter``); pass ``.t()`` of it as ``cache_keys``."""
        w = torch.load(_weight_path(cache_dir, shots), map_location="cpu", weights_only=True)
        if not isinstance(w, torch.Tensor) or w.dim() != 2:
            raise ValueError(f"{_weight_path(cache_dir, shots)} does not hold a 2-D tensor")
        w = w.detach()
        return w if device is None else w.to(device)


# ---------------------------------------------------------------------- the (beta, alpha) grid search (csrc/tip_grid.hip)
_CACHE_BUDGET_BYTES = 256 << 20          # of `cache` [beta_chunk,N,C] fp32 per call; the default beta_chunk follows from it
_CRITERIA = ("threshold_f1", "macro_f1", "accuracy")


class TipGrid:
    """What ``tip_adapter_grid`` returns.  ``betas`` [nb], ``alphas`` [na] fp32 as the device read them; the floating-point
    stage ``L0`` [N,C] and ``cache`` [nb,N,C] fp32 (``cache`` is None with ``keep_cache=False``); and, as exact functions of
    the logits ``L0 + cache[b] * alphas[a]`` (fp32, the multiply and the add rounded once each) widened to fp64:
    ``conf`` [nb,na,C,C] int32 indexed [target, pred]; ``f1``, ``threshold`` [nb,na,C] fp64; ``tp``, ``fp``, ``fn``,
    ``num_vals`` [nb,na,C] int32.  ``status``: bit 0 = a label outside [0,C) was met (such rows took no part)."""

    def __init__(self, betas, alphas, L0, cache, conf, f1, threshold, tp, fp, fn, num_vals, status):
        self.betas, self.alphas, self.L0, self.cache = betas, alphas, L0, cache
        self.conf, self.f1, self.threshold, self.tp, self.fp, self.fn, self.num_vals = conf, f1, threshold, tp, fp, fn, num_vals
        self.status = int(status)

    def logits(self, b: int, a: int) -> torch.Tensor:
        """The fp32 logits [N,C] of grid point (b, a), bit for bit what the counts were taken from."""
        if self.cache is None:
            raise RuntimeError("the cache term was not kept (keep_cache=False)")
        return self.L0 + self.cache[b] * self.alphas[a]

    def macro_f1(self) -> torch.Tensor:
        """``cls_f1`` (code/utils.py:41-76) of every grid point, [nb,na] fp64 on the CPU: the reference's formula with its
        1e-6, evaluated in fp64 from the confusion counts (the reference rounds the same expression in fp32)."""
        conf = self.conf.cpu().double()
        tp = conf.diagonal(dim1=-2, dim2=-1)
        fp, fn = conf.sum(dim=-2) - tp, conf.sum(dim=-1) - tp
        eps = 1e-6
        precision, recall = tp / (tp + fp + eps), tp / (tp + fn + eps)
        return (2 * (precision * recall) / (precision + recall + eps)).mean(dim=-1) * 100

    def accuracy(self, exclude_class: Optional[int] = None) -> torch.Tensor:
        """Top-1 ``cls_acc`` (code/utils.py:15-39) in percent, [nb,na] fp64 on the CPU; rows whose target is
        ``exclude_class`` are left out, and a grid with no row left scores 0.0."""
        conf = self.conf.cpu().double()
        correct, rows = conf.diagonal(dim1=-2, dim2=-1).clone(), conf.sum(dim=-1)
        if exclude_class is not None and 0 <= int(exclude_class) < correct.shape[-1]:
            correct[..., int(exclude_class)] = 0
            rows[..., int(exclude_class)] = 0
        valid = rows.sum(dim=-1)
        return torch.where(valid > 0, 100 * correct.sum(dim=-1) / valid.clamp(min=1), torch.zeros_like(valid))

    def threshold_f1(self, classes=None) -> torch.Tensor:
        """The mean of the best threshold F1 over ``classes`` (default: all), summed in list order as the reference's
        ``f1 += find_thresholds(...)`` loop does; [nb,na] fp64 on the CPU."""
        f1 = self.f1.cpu()
        classes = list(range(f1.shape[-1])) if classes is None else [int(c) for c in classes]
        if not classes:
            raise ValueError("threshold_f1 needs at least one class")
        total = torch.zeros(f1.shape[:-1], dtype=torch.float64)
        for c in classes:
            total = total + f1[..., c]
        return total / float(len(classes))

    def scores(self, criterion: str = "threshold_f1", classes=None) -> torch.Tensor:
        if criterion == "threshold_f1":
            return self.threshold_f1(classes)
        if criterion == "macro_f1":
            return self.macro_f1()
        if criterion == "accuracy":
            return self.accuracy()
        raise ValueError(f"criterion must be one of {_CRITERIA}, got {criterion!r}")

    def best(self, criterion: str = "threshold_f1", classes=None):
        """-> (b, a, score) by the reference's rule: beta-major order, the first score strictly above every earlier one
        wins, starting from 0.0; (None, None, 0.0) when nothing beats 0.  NaN never wins."""
        return pick_best(self.scores(criterion, classes))


def pick_best(scores: torch.Tensor):
    """The loop of code/utils.py:172-198 over a [nb,na] score table."""
    flat = scores.reshape(-1).double()
    flat = torch.where(torch.isnan(flat), torch.full_like(flat, -math.inf), flat)
    if flat.numel() == 0 or not float(flat.max()) > 0.0:
        return None, None, 0.0
    i = int((flat == flat.max()).to(torch.int8).argmax())          # the first index at the maximum
    return i // scores.shape[1], i % scores.shape[1], float(flat[i])


def tip_adapter_grid(features: torch.Tensor, labels: torch.Tensor, clip_weights: torch.Tensor, cache_keys, cache_values,
                     betas, alphas, *, adapter=None, beta_chunk: Optional[int] = None, keep_cache: bool = True) -> TipGrid:
    """Every grid point of the reference's ``search_hp`` in one device call per chunk of beta (three launches each).

    ``features`` [N,E] and ``clip_weights`` [E,C] share one dtype (bf16, fp16 or fp32); ``cache_keys`` [E,S] in that dtype, or
    ``adapter`` -- a ``TipAdapterF`` or its fp32 weight [S,E] -- in its place; ``cache_values`` [S,C]; ``labels`` [N] int64;
    ``betas`` and ``alphas`` are rounded to fp32.  ``beta_chunk`` betas are processed per call (default: as many as keep the
    call's ``cache`` [beta_chunk,N,C] within 256 MiB); with ``keep_cache=False`` only that much of the cache term is ever
    allocated and ``TipGrid.cache`` is None.  Every output is bit-identical for every chunking.  Reads the status word once
    at the end: a class whose ``num_vals`` exceeds the cap (MMR_TIP_GRID_MAX_VALS) raises a RuntimeError naming the point.
    """
    if isinstance(adapter, TipAdapterF):
        keys_t = adapter.weight
    elif adapter is not None:
        keys_t = adapter
        if not isinstance(keys_t, torch.Tensor) or keys_t.dim() != 2 or keys_t.dtype != torch.float32:
            raise ValueError("adapter must be a TipAdapterF or its fp32 weight [S,E]")
    else:
        if not isinstance(cache_keys, torch.Tensor) or cache_keys.dim() != 2:
            raise ValueError("cache_keys must be a 2-D tensor [E,S] (or pass adapter=)")
        keys_t = None
    for name, x in (("features", features), ("clip_weights", clip_weights), ("cache_values", cache_values)):
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or not x.is_floating_point():
            raise ValueError(f"{name} must be a 2-D floating-point tensor")
    N, E = features.shape
    C = clip_weights.shape[1]
    S = keys_t.shape[0] if keys_t is not None else cache_keys.shape[1]
    key_E = keys_t.shape[1] if keys_t is not None else cache_keys.shape[0]
    if clip_weights.shape[0] != E or key_E != E or tuple(cache_values.shape) != (S, C):
        raise ValueError(f"shape mismatch: features {tuple(features.shape)} [N,E], clip_weights {tuple(clip_weights.shape)} "
                         f"[E,C], keys [E={key_E},S={S}], cache_values {tuple(cache_values.shape)} [S,C]")
    if E not in _WIDTHS or not 1 <= C <= _C_MAX or not 1 <= S <= _S_MAX:
        raise ValueError(f"E={E} must be one of {_WIDTHS}, 1 <= C={C} <= {_C_MAX}, 1 <= S={S} <= {_S_MAX}")
    dt = features.dtype
    if dt not in _NATIVE_DTYPES or clip_weights.dtype != dt or (keys_t is None and cache_keys.dtype != dt):
        raise ValueError(f"features, clip_weights and cache_keys must share one of float32, bfloat16, float16 (got "
                         f"{features.dtype}, {clip_weights.dtype}, {None if keys_t is not None else cache_keys.dtype})")
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.shape[0] != N or labels.dtype != torch.int64:
        raise ValueError(f"labels must be int64 [N] = [{N}]")
    betas_t = torch.as_tensor(betas, dtype=torch.float64).reshape(-1).to(torch.float32)
    alphas_t = torch.as_tensor(alphas, dtype=torch.float64).reshape(-1).to(torch.float32)
    nb, na = betas_t.numel(), alphas_t.numel()
    if N < 1 or nb < 1 or na < 1 or nb > 65535 or na > 65535:
        raise ValueError(f"the grid needs rows and 1..65535 betas and alphas (N={N} nb={nb} na={na})")
    if beta_chunk is None:
        beta_chunk = max(1, min(nb, _CACHE_BUDGET_BYTES // (4 * N * C)))
    beta_chunk = int(beta_chunk)
    if beta_chunk < 1:
        raise ValueError(f"beta_chunk={beta_chunk} must be >= 1")
    beta_chunk = min(beta_chunk, nb)
    if not features.is_cuda:
        raise RuntimeError("features must live on the GPU (there is no CPU path)")
    dev = features.device
    f, y = features.contiguous(), labels.to(dev).contiguous()
    wct = clip_weights.to(dev).t().contiguous()
    kt = keys_t.to(dev).contiguous() if keys_t is not None else cache_keys.to(dev).t().contiguous()
    v = cache_values.to(dev, torch.float32).contiguous()
    betas_d, alphas_d = betas_t.to(dev), alphas_t.to(dev)

    i32 = dict(dtype=torch.int32, device=dev)
    L0 = torch.empty(N, C, dtype=torch.float32, device=dev)
    cache = torch.empty(nb if keep_cache else beta_chunk, N, C, dtype=torch.float32, device=dev)
    conf = torch.empty(nb, na, C, C, **i32)
    f1, thr = (torch.empty(nb, na, C, dtype=torch.float64, device=dev) for _ in range(2))
    tp, fp, fn, nv = (torch.empty(nb, na, C, **i32) for _ in range(4))
    status = torch.zeros(1, **i32)
    L = _lib.lib()
    need = L.mmr_tip_adapter_grid_workspace_bytes(N, E, C, S, beta_chunk, na)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    for b0 in range(0, nb, beta_chunk):
        n = min(beta_chunk, nb - b0)
        _lib.check(L.mmr_tip_adapter_grid(
            f.data_ptr(), y.data_ptr(), _lib.dtype_code(dt), N, E, C, S, wct.data_ptr(), kt.data_ptr(),
            _lib.dtype_code(kt.dtype), v.data_ptr(), betas_d[b0:].data_ptr(), n, alphas_d.data_ptr(), na, L0.data_ptr(),
            (cache[b0:] if keep_cache else cache).data_ptr(), conf[b0:].data_ptr(), f1[b0:].data_ptr(), thr[b0:].data_ptr(),
            tp[b0:].data_ptr(), fp[b0:].data_ptr(), fn[b0:].data_ptr(), nv[b0:].data_ptr(), status.data_ptr(), _lib.ptr(ws),
            need, _lib.stream_ptr(dev)))
    st = int(status.item())                                           # the call's one read-back
    if st & 2:
        cap = _lib.HEADER.constants["MMR_TIP_GRID_MAX_VALS"]
        b, a, c = (int(i) for i in (nv > cap).nonzero()[0])
        raise RuntimeError(f"tip_adapter_grid: grid point (b={b}, a={a}) = (beta {float(betas_t[b])!r}, alpha "
                           f"{float(alphas_t[a])!r}), class {c}: num_vals = {int(nv[b, a, c])} thresholds exceed the cap of {cap}")
    return TipGrid(betas_d, alphas_d, L0, cache if keep_cache else None, conf, f1, thr, tp, fp, fn, nv, st)


def search_lists(cfg):
    """The reference's two lists (code/utils.py:163-164), in Python floats."""
    scale, step = cfg["search_scale"], cfg["search_step"]
    return ([i * (scale[0] - 0) / step[0] + 0.01 for i in range(step[0])],
            [i * (scale[1] - 0) / step[1] + 0.01 for i in range(step[1])])


def search_hp(cfg, cache_keys, cache_values, features, labels, clip_weights, adapter=None, classes=None,
              criterion: str = "threshold_f1"):
    """The reference's ``search_hp`` (code/utils.py:159-206): with ``cfg["search_hp"]`` true, score the grid
    ``search_lists(cfg)`` (rounded to fp32 for the device) and return the winning (beta, alpha) as the unrounded list
    values, or (0, 0) when nothing beats 0; otherwise ``(cfg["init_beta"], cfg["init_alpha"])``.  ``classes=None``: every
    class but the last (the reference skips "others", its last class)."""
    if not cfg["search_hp"]:
        return cfg["init_beta"], cfg["init_alpha"]
    beta_list, alpha_list = search_lists(cfg)
    grid = tip_adapter_grid(features, labels, clip_weights, cache_keys, cache_values, beta_list, alpha_list, adapter=adapter,
                            keep_cache=False)
    if classes is None:
        classes = list(range(grid.f1.shape[-1] - 1)) or [0]
    b, a, _ = grid.best(criterion, classes)
    return (0, 0) if b is None else (beta_list[b], alpha_list[a])
