"""CPU stand-ins for gym_amd.ops with the quantised outer step -- TEST INFRASTRUCTURE.

Everything in tests/fake_outer_adam_ops.py (fake_ops plus the masked and Adam outer
steps), plus `quant_row_bytes`, `quant_encode` and `diloco_outer_dequant` as
tests/quant_checks.py states them, and recording wrappers of the unquantised
outer steps, so a test can ask which launches a run made.  A module of its own
that never sets an attribute on fake_ops.
"""
import torch

import fake_ops
import fake_outer_adam_ops as _foa
import quant_checks as Q
from fake_outer_adam_ops import *  # noqa: F401,F403
from fake_ops import _2d, _np

# every outer-step launch, in order: ("outer", K, n) | ("masked", K, n) | ("encode", K, n, bits, feedback)
# | ("dequant", S, n, bits, K_out)
CALLS = []


def diloco_outer(src, master, mom, dst, n, divisor, lr, momentum, dampening, weight_decay, nesterov, first_step):
    CALLS.append(("outer", _2d(src).shape[0], int(n)))
    fake_ops.diloco_outer(src, master, mom, dst, n, divisor, lr, momentum, dampening, weight_decay, nesterov,
                          first_step)


def diloco_outer_masked(reps, bits, master, mom, n, sparse_divisor, divisor, lr, momentum, dampening, weight_decay,
                        nesterov, first_step):
    CALLS.append(("masked", _2d(reps).shape[0], int(n)))
    _foa.diloco_outer_masked(reps, bits, master, mom, n, sparse_divisor, divisor, lr, momentum, dampening,
                             weight_decay, nesterov, first_step)


def quant_row_bytes(n, bits):
    if n < 0 or bits not in Q.QMAX:
        raise ValueError(f"quant_row_bytes: n={n} must be >= 0 and bits={bits} 4 or 8")
    return Q.row_bytes(n, bits)


def quant_encode(x, master, residual, payload, n, bits):
    x2 = _2d(x)
    K, n = x2.shape[0], int(n)
    CALLS.append(("encode", K, n, int(bits), residual is not None))
    if payload.dtype != torch.uint8 or payload.shape[0] != K or payload.shape[1] < Q.row_bytes(n, bits):
        raise ValueError("quant_encode: bad payload")
    R = _np(_2d(residual))[:, :n] if residual is not None else None
    pay, new_r, _ = Q.encode(_np(master)[:n], _np(x2)[:, :n], R, bits)
    payload[:, :pay.shape[1]] = torch.from_numpy(pay)
    if residual is not None:
        _2d(residual)[:, :n] = torch.from_numpy(new_r)


def diloco_outer_dequant(payload, master, mom, dst, n, bits, divisor, lr, momentum, dampening, weight_decay, nesterov,
                         first_step):
    n = int(n)
    d2 = _2d(dst) if dst is not None else None
    CALLS.append(("dequant", payload.shape[0], n, int(bits), 0 if d2 is None else d2.shape[0]))
    if master.dtype != torch.float32 or (mom is not None and mom.dtype != torch.float32):
        raise TypeError("diloco_outer_dequant: master and momentum must be float32")
    hp = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
    nm, nb, _ = Q.decode_outer(payload.numpy(), n, bits, divisor, _np(master)[:n],
                               None if mom is None else _np(mom)[:n], hp, bool(first_step))
    master[:n].copy_(torch.from_numpy(nm))
    if mom is not None and nb is not None:
        mom[:n].copy_(torch.from_numpy(nb))
    if d2 is not None:
        for j in range(d2.shape[0]):
            d2[j, :n].copy_(torch.from_numpy(nm).to(d2.dtype))


def install():
    """fake_ops.install(), with every gym_amd module it pointed at fake_ops pointed
    at this module instead."""
    import sys
    fake_ops.install()
    me = sys.modules[__name__]
    for name, mod in list(sys.modules.items()):
        if name.startswith("gym_amd") and getattr(mod, "ops", None) is fake_ops:
            mod.ops = me
