"""Yardsticks for the fused clip + Adam/AdamW update (no tests here).

reference_adamw is the update in numpy float64 from fp32 inputs: the per-group
clip exactly as the kernels state it, then torch.optim.AdamW's arithmetic.
torch_adamw_fp32 runs clip_grad_norm_ + torch.optim.AdamW in fp32 on the CPU
on the same inputs; its error against the float64 reference is the unit the
GPU tests measure the kernels in (check_rule).

The C ABI carries every hyper-parameter as an fp32 value, so the tests round
theirs to fp32 first (f32) and hand the reference, torch and the kernel the
same numbers: 1 - float32(0.999) differs from 1 - 0.999 by 1.3e-5 relative,
which is a different (equally valid) beta2, not a rounding error of the
update.
"""
import numpy as np
import torch


def f32(x):
    """The fp32 value nearest x, as a Python float (inf stays inf)."""
    return float(np.float32(x))


def reference_adamw(p, g, m, v, t, lr, betas, eps, wd, goff, scale, max_norm):
    """One clip + AdamW update number t >= 1 in float64; returns p, g, m, v
    (g: the clipped gradient, as the kernels leave it)."""
    p, g, m, v = (np.asarray(x).astype(np.float64).reshape(-1) for x in (p, g, m, v))  # fp32 inputs: exact
    b1, b2 = float(betas[0]), float(betas[1])
    g = g.copy()
    for lo, hi in zip(goff[:-1], goff[1:]):
        lo, hi = int(lo), int(hi)
        norm = np.sqrt(np.sum(g[lo:hi] * g[lo:hi]))
        mult = scale * min(max_norm / (norm * scale + 1e-6), 1.0)
        g[lo:hi] *= mult
    if wd != 0:
        p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** t)
    inv_sqrt_bc2 = 1.0 / np.sqrt(1.0 - b2 ** t)
    p = p - step_size * m / (np.sqrt(v) * inv_sqrt_bc2 + eps)
    return p, g, m, v


def torch_adamw(p, g, m, v, t, lr, betas, eps, wd, goff, scale, max_norm, dtype):
    """clip_grad_norm_ per group + torch.optim.AdamW (CPU, `dtype`) for update
    number t from the given state; returns p, g, m, v as float64 numpy."""
    tp, tg, tm, tv = (torch.from_numpy(np.asarray(x, dtype=np.float32).reshape(-1).copy()).to(dtype)
                      for x in (p, g, m, v))
    params = []
    for lo, hi in zip(goff[:-1], goff[1:]):
        q = tp[int(lo):int(hi)].clone().requires_grad_(True)
        q.grad = tg[int(lo):int(hi)].clone() * scale
        params.append(q)
    opt = torch.optim.AdamW(params, lr=lr, betas=tuple(betas), eps=eps, weight_decay=wd, foreach=False)
    for q, lo, hi in zip(params, goff[:-1], goff[1:]):
        opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": tm[int(lo):int(hi)].clone(),
                        "exp_avg_sq": tv[int(lo):int(hi)].clone()}
        if q.numel():
            torch.nn.utils.clip_grad_norm_([q], max_norm)
    opt.step()

    def cat(xs):
        return torch.cat([x.detach().reshape(-1) for x in xs]).double().numpy()

    return (cat(params), cat([q.grad for q in params]), cat([opt.state[q]["exp_avg"] for q in params]),
            cat([opt.state[q]["exp_avg_sq"] for q in params]))


def check_rule(what, got, ref, tor, figures=None, factor=4.0):
    """The tolerance rule of the GPU tests: with e_torch the largest error of
    fp32 torch (tor) against the float64 reference (ref), the kernel's largest
    error must stay within 4 * e_torch + 2^-23 * max|ref|.  The observed ratio
    err / e_torch goes into the message (and into `figures`).  `factor`: the 4
    of the rule, for a caller that states why its case needs another."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    assert np.all(np.isfinite(got)), f"{what}: NaN or Inf"
    err = float(np.max(np.abs(got - ref))) if got.size else 0.0
    e_torch = float(np.max(np.abs(tor - ref))) if got.size else 0.0
    bound = factor * e_torch + 2.0 ** -23 * (float(np.max(np.abs(ref))) if got.size else 0.0)
    ratio = err / e_torch if e_torch > 0 else (0.0 if err == 0 else float("inf"))
    msg = f"{what}: err {err:.3e}, e_torch {e_torch:.3e}, err/e_torch {ratio:.2f}, bound {bound:.3e}"
    print(msg)
    if figures is not None:
        figures.append((what, err, e_torch, ratio, bound))
    assert err <= bound, msg
    return ratio
