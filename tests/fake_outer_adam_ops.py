"""CPU stand-ins for gym_amd.ops with the Adam outer step -- TEST INFRASTRUCTURE.

Everything in tests/fake_ops.py, plus `diloco_outer_adam` and
`diloco_outer_adam_masked` (and the SGD `diloco_outer_masked` of
tests/fake_sparta_diloco_ops.py): ga_diloco_outer_adam's arithmetic as the
oracle states it -- oracle.reduce.mean_reduce, an fp32 subtract, then the
element update of fake_ops._adam_one (oracle/optim.py's order).  A module of its
own that never sets an attribute on fake_ops: tests in the same process rely on
a kernel layer without these ops (fused_adam_hparams' hasattr rule).
"""
import numpy as np
import torch

from fake_ops import *  # noqa: F401,F403
from fake_ops import _2d, _adam_one, _mask_bits, _np
from fake_sparta_diloco_ops import diloco_outer_masked  # noqa: F401
from oracle import reduce as oreduce

CALLS = []  # ("plain" | "masked", n, selected count) of every Adam outer step, in order


def _adam_outer(src, master, exp_avg, exp_avg_sq, dst, n, divisor, scalars):
    avg = oreduce.mean_reduce(list(_np(_2d(src))[:, :n]), divisor=divisor)
    g = torch.from_numpy((_np(master)[:n] - avg).astype(np.float32))
    _adam_one(master[:n], g, exp_avg[:n], exp_avg_sq[:n], coef=None, **scalars)
    if dst is not None:
        d2 = _2d(dst)
        for j in range(d2.shape[0]):
            d2[j, :n].copy_(master[:n].to(d2.dtype))


def diloco_outer_adam(src, master, exp_avg, exp_avg_sq, dst, n, divisor, **scalars):
    for t in (master, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32:
            raise TypeError("diloco_outer_adam: master, exp_avg and exp_avg_sq must be float32")
    CALLS.append(("plain", int(n), 0))
    _adam_outer(src, master, exp_avg, exp_avg_sq, dst, n, divisor, scalars)


def diloco_outer_adam_masked(reps, bits, master, exp_avg, exp_avg_sq, n, sparse_divisor, divisor, **scalars):
    CALLS.append(("masked", int(n), int(_mask_bits(bits, n).sum())))
    sparta_average_local(reps, n, sparse_divisor, mask=bits)  # noqa: F405
    _adam_outer(reps, master, exp_avg, exp_avg_sq, reps, n, divisor, scalars)


def install():
    """fake_ops.install(), with every gym_amd module it pointed at fake_ops
    pointed at this module instead (the same stand-ins plus the Adam outer step)."""
    import sys

    import fake_ops
    fake_ops.install()
    me = sys.modules[__name__]
    for name, mod in list(sys.modules.items()):
        if name.startswith("gym_amd") and getattr(mod, "ops", None) is fake_ops:
            mod.ops = me
