"""Expected results and designed masks for the SPARTA kernel tests (numpy and torch on
the CPU only; pinned by tests/test_sparta_checks.py).

Replica sets are [K, n] float32 arrays here (row k = replica k), whatever layout the
kernel under test takes.  Every sum is oracle.reduce.mean_reduce's: ascending replica
order, fp32 accumulation, then a true fp32 division (numpy keeps subnormals).
"""
import numpy as np
import torch

from oracle.reduce import mean_reduce


def bf16_round(x):
    """fp32 -> bf16 -> fp32, round to nearest even (torch's CPU conversion)."""
    a = np.array(x, dtype=np.float32)          # a writable copy: torch.from_numpy refuses read-only arrays
    return torch.from_numpy(a).to(torch.bfloat16).float().numpy()


def round_to(x, dtype):
    """x as the arena dtype holds it (RN_dtype), returned as float32."""
    if dtype == torch.float32:
        return np.array(x, dtype=np.float32)
    assert dtype == torch.bfloat16, dtype
    return bf16_round(x)


def _selected(mask):
    return np.flatnonzero(np.asarray(mask).reshape(-1))


def expect_fused(x, mask, divisor, dtype):
    """The one-pass average (ga_sparta_average_local): the replicas after selected
    elements of every replica <- RN_dtype(fp32_sum / divisor).  The inputs are first
    rounded to dtype; one rounding of the quotient."""
    xd = round_to(x, dtype)
    sel = _selected(mask)
    out = xd.copy()
    if sel.size:
        out[:, sel] = round_to(mean_reduce(list(xd[:, sel]), divisor), dtype)[None, :]
    return out


def expect_two_step(x, mask, divisor, dtype):
    """The exchange path (ga_sparta_select then ga_sparta_scatter): (vals, replicas)
    with vals = RN_dtype(fp32_sum) in ascending element order and selected elements
    <- RN_dtype(float(vals) / divisor).  For bf16 this rounds twice by design."""
    xd = round_to(x, dtype)
    sel = _selected(mask)
    out = xd.copy()
    if not sel.size:
        return np.zeros(0, np.float32), out
    vals = round_to(mean_reduce(list(xd[:, sel]), 1.0), dtype)
    out[:, sel] = round_to((vals / np.float32(divisor)).astype(np.float32), dtype)[None, :]
    return vals, out


def mask_with_tile_counts(counts, tile, tail, seed=0):
    """A bool mask of len(counts) * tile + tail elements: tile t holds exactly
    counts[t] selections (its first and last element among them when counts[t] >= 2,
    the rest from a seeded generator), the `tail` elements are all selected."""
    rng = np.random.default_rng(seed)
    m = np.zeros(len(counts) * tile + tail, dtype=bool)
    for t, c in enumerate(counts):
        c = int(c)
        assert 0 <= c <= tile, (t, c, tile)
        seg = m[t * tile:(t + 1) * tile]
        if c >= 2:
            seg[0] = seg[tile - 1] = True
            if c > 2:
                seg[1 + rng.choice(tile - 2, size=c - 2, replace=False)] = True
        elif c == 1:
            seg[rng.integers(tile)] = True
    m[len(counts) * tile:] = True
    return m


def bits_of(a):
    """uint32 image of a float32 array (bitwise comparisons: -0 != +0, NaN == NaN)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
