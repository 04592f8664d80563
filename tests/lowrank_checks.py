"""The low-rank (PowerSGD) outer step of include/gym_amd.h in numpy, phase by phase, with a
dtype argument: float64 is the reference, float32 the restatement whose own deviation from
float64 scales the tolerance of the orthonormalisation and of whole engine steps.  And the
first-order error bounds the GPU tests assert, written as tests/drift_bounds.py writes them.

Bounds (U = 2^-24, r the rank, K the local rows, L = ga_lowrank_chain of the walked length,
c = L + 16).  M_k = (master - x_k) + e_k is two rounded operations on values of magnitude
at most S_k = |master| + |x_k| + |e_k|: |fl(M_k) - M_k| <= 2 U S_k; the ascending sum over K
rows adds at most K U sum_k S_k.  A product entry is an fp32 chain of at most L fused
multiply-adds and at most 16 further additions (the four waves), c U sum |M| |Q| to first
order, and |M| <= sum_k S_k:
  project       (c + K + 2) U (sum_k S_k) @ |Q|
  back-project  (c + K + 2) U (sum_k S_k)^T @ |P^|
  decode        g = sum_c P^[i,c] Q[j,c] is an fmaf chain of r terms, and Q = B / K_total one
                more rounding of every term: (r + 2) U |P^| @ |Q|^T
  residual      e_k = M_k - g: the g bound, 2 U S_k for M_k, one rounding of the difference
                (|M_k - g| <= S_k + |g|, |g| within the g bound of the data): 4 U S_k
  master, mom   the update is linear in g: the g bound through its coefficients ((1 - dampening)
                into the buffer, 1 + momentum (Nesterov) or the buffer's into the step, lr into
                master), plus 8 U of the magnitudes of the terms of each result (at most four
                rounded operations, each on partial sums of those terms).
"""
import numpy as np

U = 2.0 ** -24


def views(plan, flat, which):
    """{t: the m x n matrix (which = "x"), m x r P_t ("p") or n x r Q_t ("q")} of a flat buffer."""
    out, r = {}, plan.rank
    for t in plan.compressed:
        off, m, n, _, poff, qoff = (int(v) for v in plan.tensors[t])
        start, shape = {"x": (off, (m, n)), "p": (poff, (m, r)), "q": (qoff, (n, r))}[which]
        out[t] = flat[..., start:start + shape[0] * shape[1]].reshape(flat.shape[:-1] + shape)
    return out


def deltas(master, X, E, dtype):
    """[K, n]: M_k = (master - x_k) + e_k."""
    return (np.asarray(master, dtype) - np.asarray(X, dtype)) + (np.asarray(E, dtype) if E is not None else dtype(0))


def absum(master, X, E):
    """sum_k S_k in float64."""
    e = np.abs(np.asarray(E, np.float64)) if E is not None else 0.0
    return (np.abs(np.asarray(master, np.float64)) + np.abs(np.asarray(X, np.float64)) + e).sum(axis=0)


def ksum(rows):
    acc = np.zeros_like(rows[0])
    for row in rows:
        acc = acc + row
    return acc


def _products(plan, master, X, E, F, out, dtype, back, split):
    """out's factors <- sum_k M_k F (back: M_k^T F); split: the sum of the K products (one
    process per node) instead of the product of the sum (K nodes in one process)."""
    M = deltas(master, X, E, dtype)
    Ms = [views(plan, m, "x") for m in (M if split else [ksum(M)])]
    Fv, Ov = views(plan, np.asarray(F, dtype), "p" if back else "q"), views(plan, out, "q" if back else "p")
    for t in plan.compressed:
        Ov[t][:] = ksum([(m[t].T if back else m[t]) @ Fv[t] for m in Ms])
    return out


def project(plan, master, X, E, Q, dtype=np.float64, split=False):
    """Buffer A: the P_t and the dense segments' ascending row sums."""
    A = _products(plan, master, X, E, Q, np.zeros(plan.a_len, dtype), dtype, False, split)
    for off, ln, aoff in plan.segments:
        A[aoff:aoff + ln] = ksum(np.asarray(X, dtype)[:, off:off + ln])
    return A


def backproject(plan, master, X, E, A, dtype=np.float64, split=False):
    return _products(plan, master, X, E, A, np.zeros(max(plan.b_len, 1), dtype), dtype, True, split)


def orthonormalize(P, dtype=np.float64):
    """CGS2 column by column; a zero or noise-level column becomes exactly 0."""
    P = np.array(P, dtype)
    for c in range(P.shape[1]):
        n0 = P[:, c] @ P[:, c]
        for _ in range(2):
            P[:, c] = P[:, c] - P[:, :c] @ (P[:, :c].T @ P[:, c])
        n2 = P[:, c] @ P[:, c]
        P[:, c] = 0 if (not n2 > 0 or n2 <= dtype(2.0 ** -40) * n0) else P[:, c] / np.sqrt(n2)
    return P


def orthonormalize_all(plan, A, dtype=np.float64):
    A = np.array(A, dtype)
    for P in views(plan, A, "p").values():
        P[:] = orthonormalize(P, dtype)
    return A


def sgd_update(g, master, mom, hp, first):
    """ga_diloco_outer's update from g on; returns (master, momentum or None)."""
    if hp["weight_decay"]:
        g = g + hp["weight_decay"] * master
    if hp["momentum"]:
        mom = g if first else hp["momentum"] * mom + (1 - hp["dampening"]) * g
        g = g + hp["momentum"] * mom if hp["nesterov"] else mom
    return master - hp["lr"] * g, (mom if hp["momentum"] else None)


def outer(plan, A, B, K_total, master, X, E, mom, hp, first, dtype=np.float64):
    """(g [n] (0 on padding behind compressed tensors), residual or None, master, momentum)."""
    A, master = np.asarray(A, dtype), np.asarray(master, dtype)
    Q = np.asarray(B, dtype) / dtype(K_total)
    g = np.zeros(plan.n, dtype)
    Pv, Qv, gv = views(plan, A, "p"), views(plan, Q, "q"), views(plan, g, "x")
    for t in plan.compressed:
        gv[t][:] = Pv[t] @ Qv[t].T
    Enew = None
    if E is not None:
        Enew, Mv = np.array(E, dtype), views(plan, deltas(master, X, E, dtype), "x")
        for t, e in views(plan, Enew, "x").items():
            e[:] = Mv[t] - gv[t]
    for off, ln, aoff in plan.segments:
        g[off:off + ln] = master[off:off + ln] - A[aoff:aoff + ln] / dtype(K_total)
    return (g, Enew) + sgd_update(g, master, None if mom is None else np.asarray(mom, dtype), hp, first)


def step(plan, master, X, E, B, q_div, mom, hp, first, dtype=np.float64, split=False):
    """One whole outer step over the K rows of X (K_total = K); returns (residual, master, momentum, B)."""
    A = orthonormalize_all(plan, project(plan, master, X, E, np.asarray(B, dtype) / dtype(q_div), dtype, split), dtype)
    Bn = backproject(plan, master, X, E, A, dtype, split)
    return outer(plan, A, Bn, len(X), master, X, E, mom, hp, first, dtype)[1:] + (Bn,)


def product_bound(plan, master, X, E, F, chain, K, back):
    """{t: bound} of the projection onto F = Q (back False) or the back-projection onto F = P^."""
    S = views(plan, absum(master, X, E), "x")
    Fv = views(plan, np.abs(np.asarray(F, np.float64)), "p" if back else "q")
    return {t: (chain(int(plan.tensors[t, 1 if back else 2]), back) + 16 + K + 2) * U
            * ((S[t].T if back else S[t]) @ Fv[t]) for t in plan.compressed}


def g_bound(plan, A, B, K_total):
    """[n]: the decode's bound on compressed elements, 0 elsewhere."""
    out = np.zeros(plan.n)
    Pv, Qv = views(plan, np.abs(np.asarray(A, np.float64)), "p"), views(plan, np.abs(np.asarray(B, np.float64)) / K_total, "q")
    for t, o in views(plan, out, "x").items():
        o[:] = (plan.rank + 2) * U * (Pv[t] @ Qv[t].T)
    return out


def update_bounds(gb, g, master, mom, hp, first):
    """(master bound, momentum bound): sgd_update on the g bound gb and on the magnitudes, then
    8 U of the magnitudes."""
    mag = dict(hp, lr=-hp["lr"])  # magnitudes add: master + lr |g|
    old = None if first or mom is None else np.abs(mom)
    (bm, bb), (mm, mb) = sgd_update(gb, 0 * gb, 0 * gb, dict(mag, weight_decay=0.0), first), \
        sgd_update(np.abs(g), np.abs(master), old, mag, first)
    return bm + 8 * U * mm, (bb + 8 * U * mb if hp["momentum"] else None)
