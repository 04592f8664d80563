"""numpy oracle of the MX fp8 / fp4 block-float DiLoCo outer step -- TEST INFRASTRUCTURE.

The contract and format of include/gym_amd.h (ga_mx_encode, ga_diloco_outer_mx).  Scaling
by the block's power of two and rounding to the element grid are done in float64 (exact
scaling, np.rint is round-to-nearest-even, the sign is kept); every other operation is one
float32 operation.  The outer update is quant_checks.outer_from_g.
"""
import numpy as np

from quant_checks import outer_from_g

f32 = np.float32
BLOCK = 32
TINY = f32(2.0 ** -100)  # blocks whose absmax is below it are sent as zeros
# bits -> (exponent bits, mantissa bits, bias, exponent of the largest element, its mantissa field in fp32)
FMT = {8: (4, 3, 7, 8, 0x600000), 4: (2, 1, 1, 2, 0x400000)}


def blocks(n):
    return -(-int(n) // BLOCK)


def e_bytes(n, bits):
    return blocks(n) * BLOCK * bits // 8


def row_bytes(n, bits):  # elements, then one scale byte per block, rounded up to 16
    return (e_bytes(n, bits) + blocks(n) + 15) // 16 * 16


def scale_bytes(amax, bits):
    """The E8M0 byte of every block from its float32 absmax (NaN where a block holds one)."""
    _, _, _, emax, mant = FMT[bits]
    u = np.ascontiguousarray(amax, f32).view(np.uint32).astype(np.int64)
    with np.errstate(invalid="ignore"):
        live = (amax >= TINY) & np.isfinite(amax)
    return np.where(live, (u >> 23) - emax + ((u & 0x7FFFFF) > mant), 0).astype(np.uint8)


def to_codes(v, bits):
    """float64 values within the element range -> element codes, round to nearest even, sign kept."""
    _, mb, bias, _, _ = FMT[bits]
    emin = 1 - bias
    a = np.abs(v)
    quantum = np.exp2(np.maximum(np.frexp(a)[1] - 1, emin) - mb)
    q = np.rint(a / quantum) * quantum
    ex = np.frexp(q)[1] - 1  # after rounding: a carry moves to the next binade
    normal = q >= 2.0 ** emin
    code = np.where(normal, ((ex.astype(np.int64) + bias) << mb) + ((q / np.exp2(ex) - 1) * 2 ** mb).astype(np.int64),
                    (q / 2.0 ** (emin - mb)).astype(np.int64))
    return (code | (np.signbit(v).astype(np.int64) << (bits - 1))).astype(np.uint8)


def from_codes(code, bits):
    """Element codes -> their float64 values."""
    eb, mb, bias, _, _ = FMT[bits]
    c = np.asarray(code, np.int64)
    ef, man = (c >> mb) & ((1 << eb) - 1), c & ((1 << mb) - 1)
    mag = np.where(ef == 0, man * 2.0 ** (1 - bias - mb), (1 + man / 2 ** mb) * np.exp2(ef - bias))
    return np.where((c >> (bits - 1)) & 1, -mag, mag)


def pack(codes, bits):
    codes = np.asarray(codes, np.uint8)
    return codes if bits == 8 else (codes[0::2] | (codes[1::2] << 4)).astype(np.uint8)


def unpack(eb, bits):
    eb = np.asarray(eb, np.uint8)
    return eb if bits == 8 else np.stack([eb & 0xF, eb >> 4], axis=1).reshape(-1)


def encode_row(master, x, residual, bits):
    """One node: dict(payload uint8 [row_bytes], codes [n], scales uint8 [nb], residual f32 [n] or None, d)."""
    d = np.asarray(master, f32) - np.asarray(x, f32)
    if residual is not None:
        d = d + np.asarray(residual, f32)
    n, nb = len(d), blocks(len(d))
    dp = np.zeros(nb * BLOCK, f32)
    dp[:n] = d
    dp = dp.reshape(nb, BLOCK)
    b = scale_bytes(np.abs(dp).max(axis=1), bits)
    live = (b != 0)[:, None]
    pow2 = np.exp2(b.astype(np.float64) - 127)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        codes = np.where(live, to_codes(np.where(live, dp.astype(np.float64) / pow2, 0.0), bits), 0).astype(np.uint8)
        dq = np.where(live, from_codes(codes, bits) * pow2, 0.0).astype(f32)
        new_r = (dp - dq).astype(f32).reshape(-1)[:n] if residual is not None else None
    row = np.zeros(row_bytes(n, bits), np.uint8)
    row[:e_bytes(n, bits)] = pack(codes.reshape(-1), bits)
    row[e_bytes(n, bits):e_bytes(n, bits) + nb] = b
    return dict(payload=row, codes=codes.reshape(-1)[:n], scales=b, residual=new_r, d=d)


def encode(master, X, R, bits):
    """Rows X [K, n] (and R [K, n] or None) -> (payload [K, row_bytes], new R or None, per-row dicts)."""
    X = np.asarray(X, f32).reshape(-1, np.asarray(X).shape[-1])
    rows = [encode_row(master, X[k], None if R is None else R[k], bits) for k in range(X.shape[0])]
    pay = np.stack([r["payload"] for r in rows])
    return pay, (np.stack([r["residual"] for r in rows]) if R is not None else None), rows


def decode_rows(payload, n, bits):
    """The values element * 2^(b - 127) of every payload row: [S, n] float32 (exact)."""
    nb, eb = blocks(n), e_bytes(n, bits)
    out = []
    for row in np.asarray(payload, np.uint8):
        v = from_codes(unpack(row[:eb], bits), bits).reshape(nb, BLOCK)
        b = row[eb:eb + nb].astype(np.float64)
        out.append(np.where(b[:, None] != 0, v * np.exp2(b - 127)[:, None], 0.0).astype(f32).reshape(-1)[:n])
    return np.stack(out)


def decode_outer(payload, n, bits, divisor, master, mom, hp, first):
    """(new master, new mom or None, g) from S payload rows in ascending row order."""
    acc = np.zeros(n, f32)
    for v in decode_rows(payload, n, bits):
        acc = acc + v
    g = (acc / f32(divisor)).astype(f32)
    nm, nb_ = outer_from_g(g, master, mom, hp, first)
    return nm, nb_, g
