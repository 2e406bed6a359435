"""Tip-Adapter-F: fine-tune the cache keys on the device (reference code/main_custom.py:148-247, `run_tip_adapter_F`).

The reference makes the cache keys learnable as ``adapter = nn.Linear(E, S)`` with ``adapter.weight = cache_keys.t()``
and trains that one matrix with ``AdamW(eps=1e-4)`` under ``CosineAnnealingLR`` for 20 epochs; the encoder is frozen.
One step is therefore closed-form arithmetic -- two small matrix products, an exponential, a softmax and an element-wise
optimizer -- and runs here as two HIP launches (csrc/tip_train.hip, ``mmr_tip_adapter_f_step``) with no autograd, no
host synchronisation and no device-to-host copy.  The master weight stays fp32 whatever the features' dtype.
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
