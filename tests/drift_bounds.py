"""ga_replica_gram_centered's float64 reference, the first-order error bounds its
tests assert, and a float32 numpy emulation of the kernel's summation order that the
CPU suite holds against those bounds before the GPU test relies on them.

Bounds (U = 2^-24, L = ga_replica_gram_chain()).  The kernel rounds the node mean m
and every centred value d_k = x_k - m once to fp32; following ga_replica_gram's
dist2 bound, 8 U sum |c| (|x| + |m|) for a product of two centred values, each of the
two is allowed 4 U M(e) with M(e) = max_k |x_k[e]| + |m[e]| (an allowance for rounding
that is independent from element to element, not the worst case of an ascending sum of
K = 32 terms, which is ~K/2 U max|x|).  Every accumulator is an fp32 chain of at most
L fused multiply-adds followed by at most 16 fp32 additions (wave reduction and the
four waves of a workgroup), (L + 16) U times the sum of the absolute summands to first
order; the sum over the workgroups is fp64.  So, for a sum of products p q the bound is
(L + 16) U sum |p q| + 4 U sum (|p| + |q|) M, and for a plain sum of p
(L + 16) U sum |p| + 4 U sum M:

  cgram_ij  p = d_i, q = d_j        mdot_k    p = m, q = d_k
  dsum_k    p = d_k                 mstat     p = q = m;  p = m
"""
import numpy as np

U = 2.0 ** -24
TILE, TILES, WAVES = 256, 16, 4
WAVE_COLS = TILE * TILES       # 4096 columns of a wave
WG_COLS = WAVE_COLS * WAVES    # 16384 columns of a workgroup


def reference_and_bounds(x, L):
    """((cgram, mdot, dsum, mstat), (their bounds)) in float64 from the values of x."""
    x = np.asarray(x, dtype=np.float64)
    K = x.shape[0]
    m = x.sum(axis=0) / K
    d = x - m
    M = np.abs(x).max(axis=0) + np.abs(m)
    ad, am = np.abs(d), np.abs(m)
    c, r = (L + 16) * U, 4 * U
    dM = (ad * M).sum(axis=1)
    ref = (d @ d.T, d @ m, d.sum(axis=1), np.array([m @ m, m.sum()]))
    bound = (c * (ad @ ad.T) + r * (dM[:, None] + dM[None, :]),
             c * (ad @ am) + r * ((am * M).sum() + dM),
             c * ad.sum(axis=1) + r * M.sum(),
             np.array([c * (m @ m) + 2 * r * (am * M).sum(), c * am.sum() + r * M.sum()]))
    return ref, bound


def plain_reference_and_bounds(x, L):
    """ga_replica_gram's (gram, rowsum, dist2) and the bounds of include/gym_amd.h and
    tests/test_gpu_node_drift.py, in float64 from the values of x."""
    x = np.asarray(x, dtype=np.float64)
    m = x.sum(axis=0) / x.shape[0]
    d = x - m
    d2 = (d * d).sum(axis=1)
    c = (L + 16) * U
    ref = (x @ x.T, x.sum(axis=1), d2)
    bound = (c * (np.abs(x) @ np.abs(x).T), c * np.abs(x).sum(axis=1),
             c * d2 + 8 * U * (np.abs(d) * (np.abs(x) + np.abs(m))).sum(axis=1))
    return ref, bound


def one_minus_corr(x):
    """1 - np.corrcoef(x) without its cancellation: for the unit vectors u of the
    centred rows, 1 - u_i.u_j = |u_i - u_j|^2 / 2, in extended precision.  float64's
    1 - np.corrcoef(x) itself is only good to ~1e-16 absolute, four digits of a
    1 - corr of 1e-12."""
    c = np.asarray(x, dtype=np.longdouble)
    c = c - c.mean(axis=1, keepdims=True)
    u = c / np.sqrt((c * c).sum(axis=1, keepdims=True))
    K = u.shape[0]
    out = np.zeros((K, K))
    for i in range(K):
        for j in range(i + 1, K):
            diff = u[i] - u[j]
            out[i, j] = out[j, i] = float(0.5 * (diff @ diff))
    return out


def pairwise_distance(x):
    """|x_i - x_j| in float64 from the differences themselves."""
    x = np.asarray(x, dtype=np.float64)
    K = x.shape[0]
    out = np.zeros((K, K))
    for i in range(K):
        for j in range(i + 1, K):
            out[i, j] = out[j, i] = np.linalg.norm(x[i] - x[j])
    return out


def _fma(a, b, c):
    # the product of two floats is exact in float64; one more rounding to float32
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _mfma_orders(K):
    """Column offsets inside a wave's 4096 in the order each MFMA accumulator takes
    them (gym_amd/csrc/stats.hip): one accumulator for K > 16, two for K <= 16."""
    t = np.arange(TILES)[:, None, None, None] * TILE
    if K > 16:  # 32x32x2: step j, MFMA e: columns 8j + e then 8j + 4 + e
        j, e, h = np.arange(32)[None, :, None, None], np.arange(4)[None, None, :, None], np.arange(2)
        return [(t + 8 * j + e + 4 * h[None, None, None, :]).reshape(-1)]
    j, g = np.arange(16)[None, :, None, None], np.arange(4)[None, None, None, :]
    return [(t + 16 * j + np.array(es)[None, None, :, None] + 4 * g).reshape(-1) for es in ((0, 2), (1, 3))]


def _lane_sums(p, q=None):
    """[..., waves] fp32 wave results of the per-lane accumulators over p * q (p if q is
    None) of shape [..., waves, 4096]: lane c takes columns 4c .. 4c + 3 of every tile
    in ascending order, then the xor-butterfly over the 64 lanes."""
    shp = p.shape[:-1]
    p = p.reshape(shp + (TILES, 64, 4))
    q = None if q is None else q.reshape(shp + (TILES, 64, 4))
    acc = np.zeros(shp + (64,), dtype=np.float32)
    for t in range(TILES):
        for e in range(4):
            acc = acc + p[..., t, :, e] if q is None else _fma(p[..., t, :, e], q[..., t, :, e], acc)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ o]
    return acc[..., 0]


def _over_waves(w):
    """[..., workgroups * 4] wave results: the four waves of a workgroup added in wave
    order in fp32, the workgroups in fp64."""
    w = w.reshape(w.shape[:-1] + (-1, WAVES))
    part = w[..., 0]
    for i in range(1, WAVES):
        part = part + w[..., i]
    return part.astype(np.float64).sum(axis=-1)


def emulate(x, L=WAVE_COLS):
    """(cgram, mdot, dsum, mstat) in float64 as the kernel computes them from a float32
    [K, n] array."""
    assert L == WAVE_COLS
    x = np.asarray(x, dtype=np.float32)
    K, n = x.shape
    pad = -n % WG_COLS
    x = np.concatenate([x, np.zeros((K, pad), dtype=np.float32)], axis=1)  # columns >= n read as 0
    s = np.zeros(x.shape[1], dtype=np.float32)
    for k in range(K):
        s = s + x[k]
    m = s / np.float32(K)
    d = (x - m).reshape(K, -1, WAVE_COLS)
    mw = m.reshape(-1, WAVE_COLS)
    nw = mw.shape[0]
    acc = []
    for order in _mfma_orders(K):
        a = np.zeros((K, K, nw), dtype=np.float32)
        for col in order:
            v = d[:, :, col]
            a = _fma(v[:, None, :], v[None, :, :], a)
        acc.append(a)
    cg = acc[0] if len(acc) == 1 else acc[0] + acc[1]
    mb = np.broadcast_to(mw, d.shape)
    return (_over_waves(cg), _over_waves(_lane_sums(mb, d)), _over_waves(_lane_sums(d)),
            np.array([_over_waves(_lane_sums(mw, mw)), _over_waves(_lane_sums(mw))]))
