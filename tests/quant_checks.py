"""numpy oracle of the int8 / int4 block-quantised DiLoCo outer step -- TEST INFRASTRUCTURE.

The contract of include/gym_amd.h (ga_quant_encode, ga_diloco_outer_dequant), one
individually rounded fp32 operation per line, on float32 arrays (numpy rounds every
float32 operation once, to nearest even, subnormals included).  The outer update's
fused multiply-adds are exact: fma32 rounds a * b + c once.

Format: 256-element blocks, nb = ceil(n / 256); a payload row is
[q: nb * 256 * bits / 8 bytes][scales: nb x fp32], rounded up to 16 bytes; int8 is
one two's-complement byte per element, int4 puts element 2j in bits 0-3 and element
2j + 1 in bits 4-7 of byte j; elements past n and the pad bytes are 0.
"""
import numpy as np

f32 = np.float32
BLOCK = 256
QMAX = {8: 127, 4: 7}
TINY = f32(2.0 ** -100)  # blocks whose absmax is below it quantise to zero


def blocks(n):
    return -(-int(n) // BLOCK)


def q_bytes(n, bits):
    return blocks(n) * BLOCK * bits // 8


def row_bytes(n, bits):
    return (q_bytes(n, bits) + 4 * blocks(n) + 15) // 16 * 16


def fma32(a, b, c):
    """fl32(a * b + c) with one rounding.  The float64 product of two float32 is exact;
    its float64 sum with c is taken with round-to-odd (TwoSum gives the rounding error:
    when the sum is inexact and its last bit even, it moves to the odd neighbour on the
    error's side), and a round-to-odd value of 53 bits rounds to 24 bits as the exact
    one does."""
    p = np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, f32).astype(np.float64), p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
    fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def pack(q, bits):
    """q: int array [nb * 256] in [-qmax, qmax] -> the q bytes of a payload row."""
    q = np.asarray(q, np.int64)
    if bits == 8:
        return q.astype(np.int8).view(np.uint8)
    nib = (q & 0xF).astype(np.uint8)
    return (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8)


def unpack(qb, bits):
    qb = np.asarray(qb, np.uint8)
    if bits == 8:
        return qb.view(np.int8).astype(np.int32)
    lo = (qb & 0xF).astype(np.int32)
    hi = (qb >> 4).astype(np.int32)
    out = np.empty(2 * len(qb), np.int32)
    out[0::2], out[1::2] = lo, hi
    return np.where(out > 7, out - 16, out)


def delta(master, x, residual=None):
    d = np.asarray(master, f32) - np.asarray(x, f32)
    if residual is not None:
        d = d + np.asarray(residual, f32)
    return d.astype(f32)


def encode_row(master, x, residual, bits):
    """One node.  Returns dict(payload uint8 [row_bytes], q int32 [n], scales f32 [nb],
    residual f32 [n] or None, d f32 [n])."""
    qmax = QMAX[bits]
    d = delta(master, x, residual)
    n, nb = len(d), blocks(len(d))
    dp = np.zeros(nb * BLOCK, f32)
    dp[:n] = d
    dp = dp.reshape(nb, BLOCK)
    amax = np.abs(dp).max(axis=1)
    live = amax >= TINY
    safe = np.where(live, amax, f32(1))
    s = np.where(live, safe / f32(qmax), f32(0)).astype(f32)
    inv = np.where(live, f32(qmax) / safe, f32(0)).astype(f32)
    q = np.clip(np.rint(dp * inv[:, None]), -qmax, qmax).astype(np.int32)
    q[~live] = 0
    deq = q.astype(f32) * s[:, None]
    new_r = (dp - deq).astype(f32).reshape(-1)[:n] if residual is not None else None
    row = np.zeros(row_bytes(n, bits), np.uint8)
    qb = q_bytes(n, bits)
    row[:qb] = pack(q.reshape(-1), bits)
    row[qb:qb + 4 * nb] = s.view(np.uint8)
    return dict(payload=row, q=q.reshape(-1)[:n], scales=s, residual=new_r, d=d)


def encode(master, X, R, bits):
    """Rows X [K, n] (and R [K, n] or None) -> (payload [K, row_bytes], new R or None, per-row dicts)."""
    X = np.asarray(X, f32).reshape(-1, np.asarray(X).shape[-1])
    rows = [encode_row(master, X[k], None if R is None else R[k], bits) for k in range(X.shape[0])]
    pay = np.stack([r["payload"] for r in rows])
    return pay, (np.stack([r["residual"] for r in rows]) if R is not None else None), rows


def dequant_rows(payload, n, bits):
    """The dequantised values float(q) * s of every payload row: [S, n] float32."""
    payload = np.asarray(payload, np.uint8)
    nb, qb = blocks(n), q_bytes(n, bits)
    out = []
    for row in payload:
        q = unpack(row[:qb], bits).astype(f32).reshape(nb, BLOCK)
        s = np.ascontiguousarray(row[qb:qb + 4 * nb]).view(f32)
        out.append((q * s[:, None]).astype(f32).reshape(-1)[:n])
    return np.stack(out)


def outer_from_g(g, master, mom, hp, first):
    """ga_diloco_outer's update from its pseudo-gradient on: (new master, new mom or None)."""
    m = np.asarray(master, f32)
    wd, mu = f32(hp["weight_decay"]), f32(hp["momentum"])
    if wd != 0:
        g = fma32(wd, m, g)
    buf = None
    if mu != 0:
        if first:
            buf = g.copy()
        else:
            buf = fma32(f32(1) - f32(hp["dampening"]), g, np.asarray(mom, f32) * mu)
        g = fma32(mu, buf, g) if hp["nesterov"] else buf
    return fma32(-f32(hp["lr"]), g, m), buf


def decode_outer(payload, n, bits, divisor, master, mom, hp, first):
    """(new master, new mom or None, g) from S payload rows in ascending row order."""
    acc = np.zeros(n, f32)
    for v in dequant_rows(payload, n, bits):
        acc = acc + v
    g = (acc / f32(divisor)).astype(f32)
    nm, nb_ = outer_from_g(g, master, mom, hp, first)
    return nm, nb_, g


def to_dtype_bits(x, bf16):
    """The bit patterns an arena of the dtype holds after storing fp32 x (int32 | int16;
    bf16: round to nearest even)."""
    u = np.asarray(x, f32).view(np.uint32)
    if not bf16:
        return u.view(np.int32)
    r = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return r.view(np.int16)


def bf16_round(x):
    """fp32 values representable in bf16 (round to nearest even)."""
    return (to_dtype_bits(x, True).view(np.uint16).astype(np.uint32) << 16).view(f32)
