"""Shared by test_tip_train_host.py and test_tip_train_gpu.py (not a test module): the Tip-Adapter-F step restated in
closed form (no autograd), the same step as the reference writes it (torch autograd + torch.optim.AdamW +
CosineAnnealingLR, code/main_custom.py:151-189) in a dtype of choice, the input recipes and the allowance rule.

The restatement, in fp64:
    A = F W^T; P = exp(beta*A - beta); L = 100 F Wc + 10 alpha P V; loss = sum_b(logsumexp(L_b) - L_b[y_b]) / B
    G = (softmax(L) - onehot(y)) / B; dA = beta P (10 alpha G V^T); g = dA^T F; pred = argmax, lowest c on a tie
    W *= 1 - lr*wd; m += (g - m)(1 - b1); v = v*b2 + (1 - b2) g g; W -= lr/(1 - b1^t) * m / (sqrt(v)/sqrt(1 - b2^t) + eps)
A row whose label lies outside [0,C) has loss_b = 0 and a zero row of G; the divisor stays B.
"""
import math

import torch

ADAMW = dict(betas=(0.9, 0.999), eps=1e-4, weight_decay=0.01)      # the reference's optimizer (torch's defaults but eps)


def cosine_lr(lr0, t, total):
    return lr0 * (1.0 + math.cos(math.pi * t / total)) / 2.0


def ulp32(x):
    """One unit in the last place of fp32 at magnitude |x| (the spacing just above the power of two below it)."""
    x = abs(float(x))
    return 2.0 ** -149 if x < 2.0 ** -126 else 2.0 ** (math.floor(math.log2(x)) - 23)


def allowance(ref32, ref64):
    """8 x (what fp32 torch deviates from fp64 on these inputs, max norm) + 1 fp32 ulp of the largest magnitude compared."""
    ref32, ref64 = torch.as_tensor(ref32).double(), torch.as_tensor(ref64).double()
    return 8.0 * float((ref32 - ref64).abs().max()) + ulp32(float(ref64.abs().max()))


def max_err(dev, ref64):
    return float((torch.as_tensor(dev).double().cpu() - torch.as_tensor(ref64).double()).abs().max())


# ------------------------------------------------------------------ inputs
def make_inputs(B, S, C, E, dtype=torch.bfloat16, seed=0, soft_values=False):
    """Class prototypes on the unit sphere; features = normalize(proto[y] + 8 randn/sqrt(E)) rounded to `dtype` (noisy
    enough that a good share of the rows is misclassified: losses of order 1 and gradients that are not all but zero);
    classifier rows = normalize(proto + 1.5 randn/sqrt(E)) in `dtype`; S cache keys drawn like features (class s % C),
    values their one-hot labels, or soft rows (a softmax of noise around the label) with soft_values."""
    g = torch.Generator().manual_seed(seed)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)
    proto = unit(torch.randn(C, E, generator=g, dtype=torch.float64))
    y = torch.randint(0, C, (B,), generator=g)
    noise = lambda n: torch.randn(n, E, generator=g, dtype=torch.float64) / math.sqrt(E)
    feats = unit(proto[y] + 8.0 * noise(B)).to(dtype)
    wct = unit(proto + 1.5 * noise(C)).to(dtype)                         # [C,E]
    ky = torch.arange(S) % C
    keys = unit(proto[ky] + 8.0 * noise(S)).to(dtype).float()           # [S,E]: adapter.weight
    values = torch.nn.functional.one_hot(ky, C).float()
    if soft_values:
        values = torch.softmax(3.0 * values + torch.randn(S, C, generator=g), dim=1).float()
    return dict(features=feats, targets=y, clip_weights=wct.t().contiguous(), cache_keys=keys.t().contiguous(),
                cache_values=values)


def as64(inp):
    """(F, y, Wc^T, V, W) of make_inputs' dictionary in fp64."""
    return (inp["features"].double(), inp["targets"], inp["clip_weights"].double().t().contiguous(),
            inp["cache_values"].double(), inp["cache_keys"].double().t().contiguous())


# ------------------------------------------------------------------ the closed-form restatement
def restate_forward_backward(F, y, WcT, V, W, alpha, beta):
    """-> loss, g [S,E], L [B,C], pred [B].  Works in the dtype of its arguments (fp64 in the tests)."""
    B, C = F.shape[0], WcT.shape[0]
    A = F @ W.t()
    P = torch.exp(beta * A - beta)
    L = 100.0 * (F @ WcT.t()) + (10.0 * alpha) * (P @ V)
    mx = L.max(dim=1, keepdim=True).values
    Z = L - mx
    ex = torch.exp(Z)
    ssum = ex.sum(dim=1, keepdim=True)
    valid = (y >= 0) & (y < C)
    yc = torch.where(valid, y, torch.zeros_like(y))
    loss_b = torch.log(ssum[:, 0]) - Z.gather(1, yc[:, None])[:, 0]
    loss_b = torch.where(valid, loss_b, torch.zeros_like(loss_b))
    loss = loss_b.sum() / B
    onehot = torch.zeros_like(L).scatter_(1, yc[:, None], 1.0)
    G = (ex / ssum - onehot) / B * valid[:, None].to(L.dtype)
    dA = beta * P * ((10.0 * alpha) * (G @ V.t()))
    g = dA.t() @ F
    pred = (L == mx).to(torch.int8).argmax(dim=1)          # the first (lowest) class at the maximum
    return loss, g, L, pred


def restate_adamw(W, m, v, g, lr, step, betas=ADAMW["betas"], eps=ADAMW["eps"], weight_decay=ADAMW["weight_decay"]):
    """torch's AdamW in its own order; `step` counts from 1.  -> new (W, m, v)"""
    b1, b2 = betas
    W = W * (1.0 - lr * weight_decay)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    W = W - (lr / (1.0 - b1 ** step)) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps)
    return W, m, v


def restate_train(batches, WcT, V, W, alpha, beta, lr0, total_steps, **adamw):
    """batches: [(F, y)].  -> dict(weight, exp_avg, exp_avg_sq, losses [n], lrs [n], grads [n])"""
    m, v = torch.zeros_like(W), torch.zeros_like(W)
    losses, lrs, grads = [], [], []
    for t, (F, y) in enumerate(batches):
        lr = cosine_lr(lr0, t, total_steps)
        loss, g, _, _ = restate_forward_backward(F, y, WcT, V, W, alpha, beta)
        W, m, v = restate_adamw(W, m, v, g, lr, t + 1, **adamw)
        losses.append(loss)
        lrs.append(lr)
        grads.append(g)
    return dict(weight=W, exp_avg=m, exp_avg_sq=v, losses=torch.stack(losses), lrs=lrs, grads=grads)


# ------------------------------------------------------------------ the reference's own arithmetic
def torch_train(batches, WcT, V, W, alpha, beta, lr0, total_steps, dtype, update=True):
    """The loop of run_tip_adapter_F on the CPU in `dtype`: nn.Linear adapter, F.cross_entropy, AdamW(eps=1e-4),
    CosineAnnealingLR.  Rows with a label outside [0,C) are left out of the sum and the divisor stays B (for valid labels
    that is cross_entropy's mean).  update=False: loss and gradient of the first batch only.
    -> dict(weight, exp_avg, exp_avg_sq, losses, lrs, grads, logits)"""
    S, E = W.shape
    C = WcT.shape[0]
    adapter = torch.nn.Linear(E, S, bias=False).to(dtype)
    adapter.weight = torch.nn.Parameter(W.to(dtype).clone())
    opt = torch.optim.AdamW(adapter.parameters(), lr=lr0, eps=ADAMW["eps"])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, total_steps)
    Wc, Vd = WcT.to(dtype).t(), V.to(dtype)
    losses, lrs, grads, logits = [], [], [], None
    for F, y in batches:
        F = F.to(dtype)
        affinity = adapter(F)
        cache_logits = ((-1) * (beta - beta * affinity)).exp() @ Vd * 10
        tip_logits = 100. * F @ Wc + cache_logits * alpha
        valid = (y >= 0) & (y < C)
        loss = torch.nn.functional.cross_entropy(tip_logits[valid], y[valid], reduction="sum") / F.shape[0]
        opt.zero_grad()
        loss.backward()
        lrs.append(opt.param_groups[0]["lr"])
        losses.append(loss.detach().clone())
        grads.append(adapter.weight.grad.detach().clone())
        if logits is None:
            logits = tip_logits.detach().clone()
        if not update:
            break
        opt.step()
        sched.step()
    st = opt.state[adapter.weight] if update else {}
    return dict(weight=adapter.weight.detach().clone(), exp_avg=st.get("exp_avg"), exp_avg_sq=st.get("exp_avg_sq"),
                losses=torch.stack(losses), lrs=lrs, grads=grads, logits=logits)
