"""ga_topk_encode and ga_diloco_outer_sparse launched on their own (gym_amd.ops) and
through DiLoCoOuterTopK, bit for bit against the numpy oracle of tests/topk_checks.py.

As in test_gpu_quant_kernels.py every buffer is longer than the kernel is told (row
stride ld > n, payload stride > row_bytes) and the rest holds a sentinel that must be
unchanged.  A chunk is 4096 elements: n = 31 is below k = 32, 4097 a whole chunk and a
1-element one, 12288 three chunks on the vector path, 12375 = 3 x 4096 + 87 the same
with a short tail on the element path.
"""
import numpy as np
import pytest
import torch

import topk_checks as T
from quant_checks import bf16_round, to_dtype_bits
from sgd_kernel_checks import DEV, SENT, Placed, host, t

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = [1, 31, 4096, 4097, 12288, 12375]
BYTE_SENT = 0xA5
HP = dict(lr=0.7, momentum=0.9, nesterov=True, dampening=0.0, weight_decay=0.0)
VARIANTS = {  # the outer variants of test_gpu_quant_kernels.py
    "nesterov": dict(HP), "momentum": dict(HP, nesterov=False), "plain": dict(HP, momentum=0.0, nesterov=False),
    "plain-wd": dict(HP, momentum=0.0, nesterov=False, weight_decay=1e-3),
    "dampening": dict(HP, nesterov=False, dampening=0.1), "nesterov-wd": dict(HP, weight_decay=1e-3),
    "dampening-wd": dict(HP, nesterov=False, dampening=0.2, weight_decay=1e-3),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Payload:
    """S payload rows of row_bytes at stride row_bytes + extra inside a BYTE_SENT-filled allocation."""

    def __init__(self, S, n, k, rows=None, extra=32):
        self.rb = T.row_bytes(n, k)
        self.buf = torch.full((S * (self.rb + extra) + 64,), BYTE_SENT, dtype=torch.uint8, device=DEV)
        self.view = self.buf[:S * (self.rb + extra)].view(S, self.rb + extra)
        if rows is not None:
            self.view[:, :self.rb] = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
        self.before = self.buf.clone()

    def rows(self):
        """The rows, after checking that nothing outside them changed."""
        now, keep = self.buf.clone(), self.before.clone()
        now[:self.view.numel()].view_as(self.view)[:, :self.rb] = 0
        keep[:self.view.numel()].view_as(self.view)[:, :self.rb] = 0
        assert torch.equal(now, keep)
        return self.view[:, :self.rb].cpu().numpy()


def data(seed, K, n):
    rng = np.random.default_rng(seed)
    master = (rng.standard_normal(n) * 0.02).astype(f32)
    return (master, (master + rng.standard_normal((K, n)) * 1e-3).astype(f32),
            (rng.standard_normal((K, n)) * 2e-4).astype(f32))


def same(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.int32), np.asarray(b, f32).view(np.int32))


def check_encode(master, X, R, k, tag, ld=None, off=0, dtype=torch.float32):
    """Launch on placed copies; payload bytes and residual bits against the oracle, inputs unchanged."""
    from gym_amd import ops
    K, n = X.shape
    ld = (n + 3) // 4 * 4 + 8 if ld is None else ld
    PX, PM = Placed(X, ld=ld, off=off, dtype=dtype), Placed(master, off=off)
    PR = Placed(R, ld=ld, off=off) if R is not None else None
    pay = Payload(K, n, k)
    ops.topk_encode(PX.rows, PM.view[:n], PR.rows if PR is not None else None, pay.view, n, k)
    got, (want, want_r) = pay.rows(), T.encode(master, X, R, k)
    assert PX.untouched() and PM.untouched() and (PR is None or PR.outside_untouched())
    bad = np.flatnonzero((got != want).reshape(-1))
    assert bad.size == 0, (tag, "payload bytes", bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])
    if R is not None:
        assert same(PR.data(), want_r), (tag, "residual")
    return got, (PR.data() if R is not None else None)


@pytest.mark.parametrize("k", [1, 32, 256])
@pytest.mark.parametrize("n", SIZES)
def test_encode_bit_exact(n, k):
    for K in (1, 3):
        master, X, R = data(1000 + n + K, K, n)
        for feedback in (False, True):
            check_encode(master, X, R if feedback else None, k, f"n={n} k={k} K={K} feedback={feedback}")


@pytest.mark.parametrize("how", ["odd-stride", "odd-base"])
def test_encode_element_path_gives_the_same_bytes(how):
    master, X, R = data(1100, 3, 12375)
    got = check_encode(master, X, R, 32, how, **(dict(ld=12375 + 5) if how == "odd-stride" else dict(off=1)))
    ref = check_encode(master, X, R, 32, "vector")
    assert np.array_equal(got[0], ref[0]) and same(got[1], ref[1])


@pytest.mark.parametrize("n", [12288, 12375])
def test_encode_bf16_rows(n):
    master, X, R = data(1200 + n, 3, n)
    check_encode(master, bf16_round(X), R, 32, f"bf16 n={n}", dtype=torch.bfloat16)
    check_encode(master, bf16_round(X), None, 32, f"bf16 element path n={n}", dtype=torch.bfloat16, off=1)


def special_chunks(k):
    """name -> (d [4096], the offsets that must be sent); master = -0 and x = -d, so d is exact."""
    rng = np.random.default_rng(11)
    z, low = np.zeros(T.CHUNK, f32), np.arange(k)
    mixed = np.where(rng.integers(0, 2, T.CHUNK) == 1, f32(0.37), f32(-0.37))
    plateau = (rng.uniform(-1, 1, T.CHUNK) * 0.1).astype(f32)
    flat = rng.choice(T.CHUNK, 200 + k - 1, replace=False)  # spread over lanes and register groups
    plateau[flat[:200]] = f32(0.5) * np.where(rng.integers(0, 2, 200) == 1, 1, -1).astype(f32)
    plateau[flat[200:]] = f32(2.0)
    one_lane = (rng.uniform(-1, 1, T.CHUNK) * 0.1).astype(f32)
    lane_at = (256 * np.arange(16)[:, None] + 4 * 37 + np.arange(4)).reshape(-1)[:min(k, 64)]  # lane 37's registers
    one_lane[lane_at] = f32(3.0)
    top = z.copy()
    top[T.CHUNK - k:] = -np.arange(1, k + 1, dtype=f32)
    den = z.copy()
    den[5::131] = f32(2.0 ** -140)
    negz = z.copy()
    negz[3] = f32(-0.0)
    inf = (rng.standard_normal(T.CHUNK) * 1e-3).astype(f32)
    inf[7], inf[4000] = np.inf, -np.inf
    return {"zero": (z, low), "equal": (mixed, low),
            "plateau": (plateau, np.sort(np.r_[flat[200:], flat[:200].min()])),
            "one-lane": (one_lane, np.sort(lane_at)),
            "top": (top, np.arange(T.CHUNK - k, T.CHUNK)),
            "denormals": (den, np.arange(5, T.CHUNK, 131)[:k]),
            "neg-zero": (negz, low), "inf": (inf, None)}


@pytest.mark.parametrize("k", [1, 32, 256])
def test_encode_special_chunks(k):
    """The oracle's bytes, and where the chunk's construction says which offsets are sent,
    those offsets.  With feedback R' is d - d at the sent offsets (+0; NaN for +/-inf, by
    the arithmetic) and d elsewhere."""
    for name, (d, sent) in special_chunks(k).items():
        for feedback in (False, True):
            neg0 = np.full((1, T.CHUNK), -0.0, f32)  # -0 - (-d) and d + -0 are d bit for bit, signed zeros too
            pay, res = check_encode(neg0[0], -d[None], neg0 if feedback else None, k,
                                    f"{name} k={k} feedback={feedback}")
            vals, idx = T.entries(pay[0], T.CHUNK, k)
            assert (np.diff(idx[0].astype(int)) > 0).all() and same(vals[0], d[idx[0]])
            if sent is not None and len(sent) == k:
                assert np.array_equal(idx[0], sent), (name, k)
            if name == "inf":
                assert {7, 4000} <= set(idx[0].tolist()) or k == 1
            if feedback:
                fin = np.isfinite(d[idx[0]])
                assert same(res[0][idx[0]][fin], np.zeros(int(fin.sum()), f32))  # +0, the sign bit clear
                assert same(np.delete(res[0], idx[0]), np.delete(d, idx[0]))


def check_decode(pay_rows, n, k, master, mom, hp, first, K_out, tag, bf16=False, extra=32):
    from gym_amd import ops
    S = pay_rows.shape[0]
    pay, PM = Payload(S, n, k, pay_rows, extra=extra), Placed(master)
    PB = Placed(mom if mom is not None else np.full(n, SENT, f32))
    PD = Placed(np.full((K_out, n), 3.5, f32), ld=(n + 3) // 4 * 4 + 8,
                dtype=torch.bfloat16 if bf16 else torch.float32)
    ops.diloco_outer_sparse(pay.view, PM.view[:n], PB.view[:n] if hp["momentum"] != 0 else None, PD.rows, n, k,
                            float(S), hp["lr"], hp["momentum"], hp["dampening"], hp["weight_decay"], hp["nesterov"],
                            first)
    torch.cuda.synchronize()
    assert torch.equal(pay.buf, pay.before) and all(p.outside_untouched() for p in (PM, PB, PD))
    wm, wb, _ = T.decode_outer(pay_rows, n, k, float(S), master, None if first else mom, hp, first)
    assert same(PM.data(), wm), (tag, "master")
    assert same(PB.data(), wb) if hp["momentum"] != 0 else PB.untouched(), (tag, "momentum")
    assert all(np.array_equal(row, to_dtype_bits(wm, bf16)) for row in PD.data_bits()), (tag, "dst rows")
    return PM.data(), PB.data()


def payload_rows(seed, S, n, k):
    """The oracle's encode of S rows that drifted from a common master in a common direction:
    several rows list the same index."""
    master, X, R = data(seed, S, n)
    X = (X + np.random.default_rng(seed).standard_normal(n) * 3e-3).astype(f32)
    pay = T.encode(master, X, R, k)[0]
    if S > 1:  # checks the inputs, not the kernel
        idx = np.concatenate([T.entries(p, n, k)[1][0] for p in pay])
        assert np.unique(idx[idx != T.NO_IDX], return_counts=True)[1].max() >= 2
    return master, pay


@pytest.mark.parametrize("S", [1, 3, 9])
@pytest.mark.parametrize("n", SIZES)
def test_decode_bit_exact(n, S):
    mom = (np.random.default_rng(n).standard_normal(n) * 1e-3).astype(f32)
    master, pay = payload_rows(2000 + n + S, S, n, 32)
    for K_out in (1, 3):
        check_decode(pay, n, 32, master, mom, HP, False, K_out, f"n={n} S={S} K_out={K_out}")


def test_decode_bf16_first_step_and_long_stride():
    n = 12375
    master, pay = payload_rows(2200, 3, n, 32)
    mom = (np.random.default_rng(4).standard_normal(n) * 1e-3).astype(f32)
    check_decode(pay, n, 32, master, mom, HP, False, 3, "bf16", bf16=True)
    gm, gb = check_decode(pay, n, 32, master, np.full(n, np.nan, f32), HP, True, 1, "first over NaN")
    assert np.isfinite(gm).all() and np.isfinite(gb).all()
    check_decode(pay, n, 32, master, mom, HP, False, 1, "stride", extra=4096)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_three_step_chain_every_outer_variant(name):
    """Encode with a residual, then decode in place over the K = 3 rows, three times on the
    device's own state; the last variant runs the same chain through DiLoCoOuterTopK."""
    from gym_amd import ops
    from gym_amd.engine import DiLoCoOuterTopK
    hp, n, K, k = VARIANTS[name], 12375, 3, 32
    master, X, _ = data(3000 + list(VARIANTS).index(name), K, n)
    mom, R = None, np.zeros((K, n), f32)
    PM, PB, PR, PX = Placed(master), Placed(np.full(n, SENT, f32)), Placed(R, ld=n + 9), Placed(X, ld=n + 9)
    pay = Payload(K, n, k)
    eng = DiLoCoOuterTopK(Local(), K, n, DEV, torch.float32, k=k, error_feedback=True, **hp)
    eng.init_master(t(master))
    ex = t(X)
    rng = np.random.default_rng(99)
    for step in range(3):
        ops.topk_encode(PX.rows, PM.view[:n], PR.rows, pay.view, n, k)
        ops.diloco_outer_sparse(pay.view, PM.view[:n], PB.view[:n] if hp["momentum"] != 0 else None, PX.rows, n, k,
                                float(K), hp["lr"], hp["momentum"], hp["dampening"], hp["weight_decay"],
                                hp["nesterov"], step == 0)
        eng(ex)
        want_pay, R = T.encode(master, X, R, k)
        master, mom, g = T.decode_outer(want_pay, n, k, float(K), master, mom, hp, step == 0)
        assert np.array_equal(pay.rows(), want_pay) and np.array_equal(eng.payload.cpu().numpy(), want_pay)
        assert same(PR.data(), R) and same(host(eng.residual), R) and R.any() and g.any(), (name, step)
        assert same(PM.data(), master) and same(host(eng.master), master), (name, step, "master")
        if hp["momentum"] != 0:
            assert same(PB.data(), mom) and same(host(eng.mom), mom), (name, step, "momentum")
        assert all(same(row, master) for row in [*PX.data(), *host(ex)]), (name, step, "rows")
        assert all(p.outside_untouched() for p in (PM, PB, PR, PX)) and (hp["momentum"] != 0 or PB.untouched())
        X = (master + rng.standard_normal((K, n)) * 1e-3).astype(f32)  # the nodes train on
        PX.rows.copy_(t(X))
        ex.copy_(t(X))


class Local:
    world, rank, exchange, rccl, backend = 1, 0, False, False, "none"


def test_fragmented_strategy_steps_both_fragments():
    """DiLoCoStrategy(num_fragments=2, outer_compression="topk") through build_streaming_outer:
    each fragment's engine takes its slice to the oracle's result, chunks restarting at its start."""
    from gym_amd.strategy import DiLoCoStrategy
    from gym_amd.strategy.diloco import build_streaming_outer
    n, K = 16384, 2
    s = DiLoCoStrategy(H=4, num_fragments=2, outer_compression="topk", outer_error_feedback=True)
    fr = build_streaming_outer(s, s.outer_optim_spec, Local(), K, n, DEV, torch.float32, [0, 5120, 9000], (2, 0, 0.0))
    master, X, _ = data(4000, K, n)
    fr.init_master(t(master))
    ex = t(X)
    for eng, a, b in zip(fr.engines, fr.bounds, fr.bounds[1:]):
        eng(ex[:, a:b])
        pay, R = T.encode(master[a:b], X[:, a:b], np.zeros((K, b - a), f32), 32)
        wm, wb, _ = T.decode_outer(pay, b - a, 32, float(K), master[a:b], None, HP, True)
        assert eng.k == 32 and same(host(eng.master), wm) and same(host(eng.residual), R)
        assert all(same(row, wm) for row in host(ex[:, a:b])) and same(host(eng.mom), wb)
    assert fr.bounds[0] == 0 and fr.bounds[-1] == n and len(fr.engines) == 2


def test_zero_length_launches_touch_nothing():
    from gym_amd import ops
    x, m = torch.full((2, 16), SENT, device=DEV), torch.full((16,), SENT, device=DEV)
    pay = torch.full((2, 16), BYTE_SENT, dtype=torch.uint8, device=DEV)
    ops.topk_encode(x, m, None, pay, 0, 32)
    ops.diloco_outer_sparse(pay, m, None, x, 0, 32, 2.0, 0.7, 0.0, 0.0, 0.0, False, True)
    assert (host(x) == SENT).all() and (host(m) == SENT).all() and (pay.cpu().numpy() == BYTE_SENT).all()
