"""CPU stand-ins for gym_amd.ops with the fused SGD step -- TEST INFRASTRUCTURE.

Everything in tests/fake_ops.py, plus `sgd_step`: ga_sgd_step's arithmetic
(gym_amd/csrc/sgd_math.h) in numpy float32, every fused multiply-add through
float64 and rounded once, as fake_ops._adam_one does."""
import numpy as np
import torch

from fake_ops import *  # noqa: F401,F403
from fake_ops import _2d, _np


def _fma(a, b, c):
    """fl32(a * b + c) of float32 operands: the product is exact in float64."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def sgd_step(param, grad, buf, *, neg_lr, momentum, one_m_dampening, weight_decay, nesterov, first, clip_coef=None,
             n=None):
    if buf is None and momentum != 0:
        raise ValueError("sgd_step: a momentum buffer is required with momentum != 0")
    P2, G2 = _2d(param), _2d(grad)
    B2 = _2d(buf) if buf is not None else None
    n = P2.shape[1] if n is None else int(n)
    f = np.float32
    for k in range(P2.shape[0]):
        p, g = _np(P2[k, :n]).copy(), _np(G2[k, :n]).copy()
        coef = None if clip_coef is None else float(clip_coef[2 * k])
        if coef is not None and not coef >= 1.0:  # a NaN coefficient scales too (ga_adam_step's rule)
            g = (g * f(coef)).astype(f)
            G2[k, :n].copy_(torch.from_numpy(g))
        if weight_decay != 0:
            g = _fma(f(weight_decay), p, g)
        if momentum != 0:
            if first:
                b = g.copy()
            else:
                b = _fma(f(one_m_dampening), g, (_np(B2[k, :n]) * f(momentum)).astype(f))
            B2[k, :n].copy_(torch.from_numpy(b))
            g = _fma(f(momentum), b, g) if nesterov else b
        P2[k, :n].copy_(torch.from_numpy(_fma(f(neg_lr), g, p)))


def install():
    """fake_ops.install(), with every gym_amd module it pointed at fake_ops
    pointed at this module instead (the same stand-ins plus sgd_step)."""
    import sys

    import fake_ops
    fake_ops.install()
    me = sys.modules[__name__]
    for name, mod in list(sys.modules.items()):
        if name.startswith("gym_amd") and getattr(mod, "ops", None) is fake_ops:
            mod.ops = me
