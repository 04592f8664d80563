"""CPU stand-ins for gym_amd.ops with the island outer step -- TEST INFRASTRUCTURE.

Everything in tests/fake_stream_ops.py, plus `diloco_outer_islands` as
tests/island_checks.py states it, recorded in the same CALLS list as the other
outer-step launches: ("islands", S, n, islands, slots, K_state, aliased).  The host
tables go through the real wrapper's checks (gym_amd.ops.island_table, which needs no
GPU).  A module of its own that never sets an attribute on the modules it builds on.
"""
import torch

import fake_stream_ops as _fs
import island_checks as I
from fake_stream_ops import *  # noqa: F401,F403
from fake_ops import _2d, _np

# fake_stream_ops' list (fake_quant_ops'): every recording wrapper appends to the same one
CALLS = _fs.CALLS


def diloco_outer_islands(src, islands, slots, master, mom, x, n, lr, momentum, dampening, weight_decay, nesterov,
                         first_step):
    from gym_amd.ops import island_table
    n = int(n)
    s2, x2, m2 = _2d(src), _2d(x), _2d(master)
    b2 = _2d(mom) if mom is not None else None
    islands = [[int(m) for m in isl] for isl in islands]
    slots = [[int(v) for v in sl] for sl in slots]
    aliased = x2.data_ptr() == s2.data_ptr()
    _fs.CALLS.append(("islands", s2.shape[0], n, islands, slots, x2.shape[0], aliased))
    island_table(islands, slots, s2.shape[0], x2.shape[0])
    if m2.dtype != torch.float32 or (b2 is not None and b2.dtype != torch.float32):
        raise TypeError("diloco_outer_islands: master and momentum must be float32")
    if x2.dtype != s2.dtype:
        raise TypeError("diloco_outer_islands: src/x dtype mismatch")
    if m2.shape[0] != x2.shape[0] or (b2 is not None and b2.shape[0] != x2.shape[0]):
        raise ValueError("diloco_outer_islands: state rows do not match x")
    if float(momentum) != 0.0 and b2 is None:
        raise ValueError("diloco_outer_islands: momentum != 0 needs a momentum buffer")
    if s2.shape[1] < n or x2.shape[1] < n or m2.shape[1] < n or (b2 is not None and b2.shape[1] < n):
        raise ValueError("diloco_outer_islands: buffers shorter than n")
    hp = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
    has_mom = float(momentum) != 0.0
    nm, nb, rows = I.step(_np(s2)[:, :n].copy(), islands, slots, _np(m2)[:, :n].copy(),
                          _np(b2)[:, :n].copy() if has_mom else None, hp, bool(first_step),
                          s2.dtype == torch.bfloat16)
    m2[:, :n] = torch.from_numpy(nm)
    if has_mom:
        b2[:, :n] = torch.from_numpy(nb)
    for slot, row in rows.items():
        x2[slot, :n] = torch.from_numpy(row).to(x2.dtype)


def install():
    """fake_stream_ops.install(), with every gym_amd module it pointed at fake_stream_ops
    pointed at this module instead."""
    import sys
    _fs.install()
    me = sys.modules[__name__]
    for name, mod in list(sys.modules.items()):
        if name.startswith("gym_amd") and getattr(mod, "ops", None) is _fs:
            mod.ops = me
