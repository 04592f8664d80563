"""Inner optimizer step (oracle; test infrastructure only).

Reference: the strategies' `clip_grad_norm_(model.parameters(), max_norm)` +
`self.optim.step()` with the default torch.optim.AdamW
(exogym/strategy/strategy.py:135-140, diloco.py:52-59,
communicate_optimize_strategy.py:69-74; OptimSpec default optim.py:11).
The arithmetic lives in torch (third party, torch 2.10 here):
torch/optim/adam.py `_multi_tensor_adam` (AdamW = decoupled weight decay)
and torch/nn/utils/clip_grad.py.  Restated in numpy fp32 in torch's op order;
`a + s*b` forms that ATen evaluates with a fused multiply-add are evaluated
exactly and rounded once.  Pinned against torch.optim.AdamW / clip_grad_norm_
run here (tests/test_oracle_golden.py).  `sgd_step` is the "sgd" inner
optimizer (torch.optim.SGD, torch/optim/sgd.py `_single_tensor_sgd`) in the same
style, pinned against torch.optim.SGD on the CPU (tests/test_oracle_sgd.py).
"""
import numpy as np

f32 = np.float32


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def clip_coef(grads, max_norm):
    """(coef, total_norm) of clip_grad_norm_ (norm type 2, eps 1e-6, clamped to 1
    as torch.clamp(max=1) does: a NaN norm gives a NaN coefficient, an infinite one 0)."""
    with np.errstate(over="ignore", invalid="ignore"):
        total = np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads))
        coef = float(f32(max_norm) / (f32(total) + f32(1e-6)))
    return (1.0 if coef >= 1.0 else coef), total


def adam_step(p, g, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=True,
              clip=None):
    """One Adam(W) step on fp32 arrays; step = the step count after increment.
    `clip` is clip_coef's coefficient: the gradient is scaled unless clip >= 1, so
    a NaN coefficient makes the whole step NaN, as clip_grad_norm_ does.
    Returns (p, g_used, m, v)."""
    with np.errstate(over="ignore", invalid="ignore"):  # non-finite gradients are part of the contract
        return _adam_step(p, g, m, v, step, lr, betas, eps, weight_decay, decoupled, clip)


def _adam_step(p, g, m, v, step, lr, betas, eps, weight_decay, decoupled, clip):
    b1, b2 = betas
    p, g, m, v = (np.asarray(x, f32).copy() for x in (p, g, m, v))
    if clip is not None and not clip >= 1.0:
        g = (g * f32(clip)).astype(f32)
    if weight_decay != 0:
        if decoupled:
            p = (p * f32(1 - lr * weight_decay)).astype(f32)
        else:
            g = _fma(f32(weight_decay), p, g)
    w = f32(1 - b1)
    d = (g - m).astype(f32)
    if w < 0.5:  # ATen's lerp: a + w*(b-a) for w < 0.5, else b - (b-a)*(1-w), each rounded once
        m = _fma(w, d, m)
    else:
        m = _fma(-d, f32(1) - w, g)
    v = (v * f32(b2)).astype(f32)
    v = _fma((f32(1 - b2) * g).astype(f32), g, v)
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    step_size = f32(-(lr / bc1))
    denom = ((np.sqrt(v).astype(f32) / f32(bc2 ** 0.5)).astype(f32) + f32(eps)).astype(f32)
    p = _fma(step_size, (m / denom).astype(f32), p)
    return p, g, m, v


def sgd_step(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first=False, clip=None):
    """One torch.optim.SGD step on fp32 arrays (torch/optim/sgd.py `_single_tensor_sgd`:
    `grad.add(param, alpha=wd)`, `buf = clone(grad)` on the parameter's first step, else
    `buf.mul_(momentum).add_(grad, alpha=1 - dampening)`, `grad.add(buf, alpha=momentum)`
    for Nesterov, `param.add_(grad, alpha=-lr)`; every `a + s*b` rounded once).  The
    scalars are rounded to fp32 once, -lr and 1 - dampening computed in double first.
    `clip` as in adam_step.  buf is not read on a first step or without momentum (it may
    be None) and comes back as given without momentum.
    Returns (p, g_left, buf): g_left is the clipped gradient, which is what stays behind."""
    with np.errstate(over="ignore", invalid="ignore"):  # non-finite gradients are part of the contract
        return _sgd_step(p, g, buf, lr, momentum, dampening, weight_decay, nesterov, first, clip)


def _sgd_step(p, g, buf, lr, momentum, dampening, weight_decay, nesterov, first, clip):
    p, g = np.asarray(p, f32).copy(), np.asarray(g, f32).copy()
    if clip is not None and not clip >= 1.0:
        g = (g * f32(clip)).astype(f32)
    g_left = g
    if weight_decay != 0:
        g = _fma(f32(weight_decay), p, g)
    if momentum != 0:
        if first:
            buf = g.copy()
        else:
            buf = _fma(f32(1 - dampening), g, (np.asarray(buf, f32) * f32(momentum)).astype(f32))
        g = _fma(f32(momentum), buf, g) if nesterov else buf
    p = _fma(f32(-lr), g, p)
    return p, g_left, buf
