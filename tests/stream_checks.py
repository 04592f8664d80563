"""numpy oracle of the streaming DiLoCo outer step -- TEST INFRASTRUCTURE.

The contract of include/gym_amd.h (ga_diloco_outer_merge), one individually rounded
fp32 operation per line, on float32 arrays (numpy rounds every float32 operation
once, to nearest even); the outer update's fused multiply-adds are quant_checks'
fma32 (one rounding).  Beside it the host side of engine.FragmentedOuter, stated
independently: where the arena is cut (bounds), when a fragment fires (fires) and a
replay of a whole run over given per-step row contents (run).
"""
import numpy as np

from quant_checks import bf16_round, fma32, outer_from_g

f32 = np.float32


def _store(x, bf16):
    """The value an arena of the dtype holds after storing fp32 x."""
    x = np.asarray(x, f32)
    return bf16_round(x) if bf16 else x


def merge(S_rows, divisor, master, mom, hp, first, alpha, X, bf16):
    """ga_diloco_outer_merge.  S_rows [K, n]: the values the source rows hold; master,
    mom [n] fp32 (mom None: momentum 0, or the first step); X [K_out, n] the values the
    live rows hold, or None (K_out = 0).  Returns (new master, new mom or None, the
    values the live rows hold afterwards [K_out, n] or None)."""
    S_rows = np.asarray(S_rows, f32)
    master = np.asarray(master, f32)
    alpha = f32(alpha)
    total = np.zeros(S_rows.shape[1], f32)
    for row in S_rows:                                   # sum = 0.f + src_0 + ... + src_{K-1}
        total = total + row
    avg = (total / f32(divisor)).astype(f32)             # avg = sum / divisor
    g = (master - avg).astype(f32)                       # g = master - avg
    m, buf = outer_from_g(g, master, mom, hp, first)     # ga_diloco_outer's update from g on
    if X is None:
        return m, buf, None
    X = np.asarray(X, f32)
    if alpha == 0:
        out = np.stack([_store(m, bf16) for _ in range(X.shape[0])]) if X.shape[0] else X.copy()
    else:
        part = ((f32(1) - alpha) * m).astype(f32)        # (1.f - alpha) * m
        out = np.stack([_store(fma32(alpha, x, part), bf16) for x in X]) if X.shape[0] else X.copy()
    return m, buf, out


def bounds(offsets, n, F, unit):
    """c_0 = 0, c_F = n; for 0 < f < F the start of the tensor nearest to f n / F (ties to
    the lower), rounded down to a multiple of unit.  None when not strictly increasing."""
    from fractions import Fraction
    out = [0]
    for f in range(1, F):
        target = Fraction(f * n, F)
        best = None
        for o in sorted(offsets):
            if best is None or abs(o - target) < abs(best - target):
                best = o
        out.append(best - best % unit)
    out.append(n)
    return out if all(a < b for a, b in zip(out, out[1:])) else None


def fires(f, step, H, F):
    """Fragment f of F sends (or, without a delay, takes its outer step) at `step`."""
    return step > 0 and (step + (f * H) // F) % H == 0


def run(X0, deltas, cuts, H, delay, alpha, hp, K_total=None, bf16=False, staged=None):
    """Replay of FragmentedOuter over K rows that start as X0 [K, n] with master = X0[0]:
    at step t every row takes deltas[t] [K, n] (the inner step: x <- store(x + delta)),
    then, fragment by fragment in ascending order, a merge due at t lands and a fragment
    that fires at t sends -- or, with delay 0, steps at once.  A sent fragment's staged
    sum is the ascending fp32 sum of its rows stored in the arena's dtype (staged: an
    exchange or a delay; otherwise the step sums the live rows in place).
    Returns one dict per step: rows [K, n], master [n], mom [n] (zeros until a
    fragment's first step), events [("send" | "merge" | "step", f)]."""
    X = _store(np.array(X0, f32), bf16)
    K, n = X.shape
    F = len(cuts) - 1
    K_total = K if K_total is None else K_total
    staged = (delay > 0) if staged is None else staged
    master = np.array(X[0], f32)
    mom = np.zeros(n, f32)
    first = [True] * F
    pending = [None] * F  # (due step, staged sum)
    has_mom = hp["momentum"] != 0
    out = []

    def land(f, src_rows):
        a, b = cuts[f], cuts[f + 1]
        m, buf, x = merge(src_rows, K_total, master[a:b], None if (first[f] or not has_mom) else mom[a:b], hp,
                          first[f], alpha, X[:, a:b], bf16)
        master[a:b] = m
        if buf is not None:
            mom[a:b] = buf
        X[:, a:b] = x
        first[f] = False

    def stage(f):
        a, b = cuts[f], cuts[f + 1]
        total = np.zeros(b - a, f32)
        for row in X[:, a:b]:
            total = total + row
        return _store(total, bf16)[None, :]

    for t, d in enumerate(deltas):
        X = _store((X + np.asarray(d, f32)).astype(f32), bf16)
        events = []
        for f in range(F):
            if pending[f] is not None and pending[f][0] == t:
                land(f, pending[f][1])
                pending[f] = None
                events.append(("merge", f))
            if fires(f, t, H, F):
                if delay == 0:
                    land(f, stage(f) if staged else X[:, cuts[f]:cuts[f + 1]].copy())
                    events.append(("step", f))
                else:
                    pending[f] = (t + delay, stage(f))
                    events.append(("send", f))
        out.append(dict(rows=X.copy(), master=master.copy(), mom=mom.copy(), events=events))
    return out
