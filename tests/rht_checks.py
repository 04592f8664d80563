"""numpy oracle of the Hadamard-rotated int8 / int4 DiLoCo outer step -- TEST INFRASTRUCTURE.

The contract of include/gym_amd.h (ga_rht_encode, ga_diloco_outer_rht), one individually
rounded fp32 operation per line on float32 arrays.  The payload row, the quantise lines
and the outer update are tests/quant_checks.py's.
"""
import numpy as np

import quant_checks as Q

f32 = np.float32
BLOCK = Q.BLOCK
M32 = 0xFFFFFFFF


def fmix32(h):
    """murmur3's 32-bit finaliser on a uint64 array holding 32-bit values."""
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def sigma(n, seed):
    """The sign diagonal of elements 0 .. n - 1: float32 +1 / -1."""
    i = np.arange(n, dtype=np.uint64)
    word = fmix32((i >> 5) + ((int(seed) * 0x9E3779B9) & M32))
    return np.where((word >> (i & 31)) & 1, f32(-1), f32(1)).astype(f32)


def fwht256(v):
    """FWHT256 of every 256 consecutive values of v, stage by stage: [nb, 256]."""
    v, h = np.asarray(v, f32).reshape(-1, BLOCK), 1
    with np.errstate(invalid="ignore", over="ignore"):
        while h < BLOCK:
            p = v.reshape(len(v), BLOCK // (2 * h), 2, h)
            a, b = p[:, :, 0, :], p[:, :, 1, :]
            v, h = np.stack([a + b, a - b], axis=2).astype(f32).reshape(-1, BLOCK), 2 * h
        return (v * f32(2.0 ** -4)).astype(f32)


def encode(master, X, R, bits, seed):
    """Rows X [K, n] (and R [K, n] or None) -> (payload [K, row_bytes], new R or None, per-row
    dicts of q int32 [nb, 256], scales f32 [nb], y f32 [nb, 256], d f32 [n])."""
    X = np.asarray(X, f32).reshape(-1, np.asarray(X).shape[-1])
    K, n = X.shape
    qmax, nb, qb = Q.QMAX[bits], Q.blocks(n), Q.q_bytes(n, bits)
    sg = sigma(nb * BLOCK, seed)
    pay, new_r, rows = np.zeros((K, Q.row_bytes(n, bits)), np.uint8), None if R is None else np.zeros((K, n), f32), []
    for k in range(K):
        with np.errstate(invalid="ignore", over="ignore"):
            d = Q.delta(master, X[k], None if R is None else R[k])
            dp = np.zeros(nb * BLOCK, f32)
            dp[:n] = d
            y = fwht256(dp * sg)
            amax = np.abs(y).max(axis=1)
            live = (amax >= Q.TINY) & np.isfinite(amax)
            safe = np.where(live, amax, f32(1))
            s = np.where(live, safe / f32(qmax), f32(0)).astype(f32)
            inv = np.where(live, f32(qmax) / safe, f32(0)).astype(f32)
            q = np.clip(np.rint(np.where(live[:, None], y, f32(0)) * inv[:, None]), -qmax, qmax).astype(np.int32)
            if R is not None:
                w = fwht256((q.astype(f32) * s[:, None]).astype(f32)).reshape(-1)
                new_r[k] = (dp - sg * w).astype(f32)[:n]
        pay[k, :qb], pay[k, qb:qb + 4 * nb] = Q.pack(q.reshape(-1), bits), s.view(np.uint8)
        rows.append(dict(q=q, scales=s, y=y, d=d))
    return pay, new_r, rows


def decode_outer(payload, n, bits, divisor, master, mom, hp, first, seed):
    """(new master, new mom or None, g) from S payload rows added in the rotated domain in
    ascending row order and rotated back once."""
    nb, qb = Q.blocks(n), Q.q_bytes(n, bits)
    acc = np.zeros((nb, BLOCK), f32)
    for row in np.asarray(payload, np.uint8):
        s = np.ascontiguousarray(row[qb:qb + 4 * nb]).view(f32)
        acc = acc + (Q.unpack(row[:qb], bits).astype(f32).reshape(nb, BLOCK) * s[:, None]).astype(f32)
    w = (sigma(nb * BLOCK, seed) * fwht256(acc).reshape(-1))[:n]
    g = (w / f32(divisor)).astype(f32)
    return (*Q.outer_from_g(g, master, mom, hp, first), g)
