"""CPU stand-ins for gym_amd.ops with the streaming outer step -- TEST INFRASTRUCTURE.

Everything in tests/fake_quant_ops.py, plus `diloco_outer_merge` as
tests/stream_checks.py states it, recorded in the same CALLS list as the other
outer-step launches: ("merge", K, n, K_out, alpha, aliased).  A module of its own
that never sets an attribute on fake_ops or fake_quant_ops.
"""
import torch

import fake_quant_ops as _fq
import stream_checks as S
from fake_quant_ops import *  # noqa: F401,F403
from fake_ops import _2d, _np

# fake_quant_ops' list: its recording wrappers and the one below append to the same one
CALLS = _fq.CALLS


def diloco_outer_merge(src, master, mom, x, n, divisor, lr, momentum, dampening, weight_decay, nesterov, first_step,
                       alpha):
    n = int(n)
    s2 = _2d(src)
    x2 = _2d(x) if x is not None else None
    aliased = x2 is not None and x2.data_ptr() == s2.data_ptr()
    _fq.CALLS.append(("merge", s2.shape[0], n, 0 if x2 is None else x2.shape[0], float(alpha), aliased))
    if master.dtype != torch.float32 or (mom is not None and mom.dtype != torch.float32):
        raise TypeError("diloco_outer_merge: master and momentum must be float32")
    if x2 is not None and x2.dtype != s2.dtype:
        raise TypeError("diloco_outer_merge: src/x dtype mismatch")
    if not 0.0 <= float(alpha) < 1.0:
        raise ValueError(f"diloco_outer_merge: alpha={alpha!r} is not in [0, 1)")
    if s2.shape[1] < n or master.numel() < n or (x2 is not None and x2.shape[1] < n):
        raise ValueError("diloco_outer_merge: buffers shorter than n")
    hp = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
    prev = None if (first_step or mom is None) else _np(mom)[:n].copy()
    nm, nb, nx = S.merge(_np(s2)[:, :n].copy(), divisor, _np(master)[:n].copy(), prev, hp, bool(first_step), alpha,
                         None if x2 is None else _np(x2)[:, :n].copy(), s2.dtype == torch.bfloat16)
    master[:n].copy_(torch.from_numpy(nm))
    if mom is not None and nb is not None:
        mom[:n].copy_(torch.from_numpy(nb))
    if x2 is not None:
        x2[:, :n] = torch.from_numpy(nx).to(x2.dtype)


def install():
    """fake_quant_ops.install(), with every gym_amd module it pointed at fake_quant_ops
    pointed at this module instead."""
    import sys
    _fq.install()
    me = sys.modules[__name__]
    for name, mod in list(sys.modules.items()):
        if name.startswith("gym_amd") and getattr(mod, "ops", None) is _fq:
            mod.ops = me
