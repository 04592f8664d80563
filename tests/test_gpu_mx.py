"""ga_mx_encode, ga_diloco_outer_mx, DiLoCoOuterMX and outer_compression="mxfp4" on the
MI355X, every byte and bit against tests/mx_checks.py, no tolerance.  A block is 32
elements, a lane owns 8, a wave 512, a workgroup 4096: the sizes are short / whole / whole +
short blocks, ends inside a wave (520 % 8 == 0: the decode's vector path) and a second
workgroup.  Buffers are longer than the kernel is told; the rest is a sentinel."""
import numpy as np
import pytest
import torch

import mx_checks as M
from quant_checks import bf16_round, to_dtype_bits
from sgd_kernel_checks import DEV, SENT, Placed

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = [1, 31, 32, 33, 511, 520, 4096 + 40]
HP = dict(lr=0.7, momentum=0.9, nesterov=True, dampening=0.0, weight_decay=1e-3)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def same(a, b):
    """Bit-identical fp32 arrays (NaNs: a NaN in the same places)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan])


def data(seed, K, n):
    """A heavy-tailed delta: 3% of the entries 100 times larger."""
    rng = np.random.default_rng(seed)
    master = (rng.standard_normal(n) * 0.02).astype(f32)
    X = (master + rng.standard_normal((K, n)) * 1e-3 * np.where(rng.random((K, n)) < 0.03, 100, 1)).astype(f32)
    return master, X, (rng.standard_normal((K, n)) * 2e-5).astype(f32)


def payload_buf(S, n, bits, rows=None):
    """S payload rows of stride row_bytes + 32 in a 0xA5-filled allocation."""
    rb = M.row_bytes(n, bits)
    buf = torch.full((S, rb + 32), 0xA5, dtype=torch.uint8, device=DEV)
    if rows is not None:
        buf[:, :rb] = torch.from_numpy(rows).to(DEV)
    return buf, rb


def check_encode(master, X, R, bits, tag, off=0, dtype=torch.float32):
    from gym_amd import ops
    K, n = X.shape
    ld = (n + 7) // 8 * 8 + 8
    PX, PM = Placed(X, ld=ld, off=off, dtype=dtype), Placed(master, off=off)
    PR = Placed(R, ld=ld, off=off) if R is not None else None
    buf, rb = payload_buf(K, n, bits)
    ops.mx_encode(PX.rows, PM.view[:n], PR.rows if PR else None, buf, n, bits)
    want, want_r, rows = M.encode(master, X, R, bits)
    got = buf.cpu().numpy()
    bad = np.flatnonzero((got[:, :rb] != want).reshape(-1))
    assert bad.size == 0, (tag, "payload", bad[:8], got[:, :rb].reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])
    assert (got[:, rb:] == 0xA5).all() and PX.untouched() and PM.untouched(), tag
    if R is not None:
        assert same(PR.data(), want_r) and PR.outside_untouched(), (tag, "residual")
    return rows


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", [8, 4])
def test_encode_bytes_and_residual(bits, n, feedback, bf16):
    for K in (1, 3):
        master, X, R = data(100 + n + K, K, n)
        X = bf16_round(X) if bf16 else X
        check_encode(master, X, R if feedback else None, bits, (bits, n, K, feedback, bf16),
                     dtype=torch.bfloat16 if bf16 else torch.float32)


@pytest.mark.parametrize("bits", [8, 4])
def test_encode_element_path(bits):
    """Every pointer one element off 16-byte alignment."""
    master, X, R = data(7, 3, 4096 + 40)
    check_encode(master, X, R, bits, "offset", off=1)
    check_encode(master, bf16_round(X), None, bits, "offset bf16", off=1, dtype=torch.bfloat16)


@pytest.mark.parametrize("bits", [8, 4])
def test_encode_special_blocks(bits):
    """Blocks built by hand (master = 0 and x = -d, so d is exact): all zero; amax just
    below and at 2^-100; a NaN and an Inf block; amax at elem_max * 2^3 and the next
    float (the scale bump); grid midpoints and a negative value that rounds to zero
    under amax = elem_max; a short tail block."""
    top, emax = (448.0, 8) if bits == 8 else (6.0, 2)
    rng = np.random.default_rng(bits)
    d = (rng.uniform(-1, 1, (9, 32)) * 2.0 ** -102).astype(f32)
    d[0] = 0
    d[1, 5], d[2, 31] = np.nextafter(f32(2.0 ** -100), f32(0)), -f32(2.0 ** -100)
    d[3], d[4] = rng.standard_normal(32), rng.standard_normal(32)
    d[3, 7], d[4, 9] = np.nan, -np.inf
    d[5], d[6] = rng.uniform(-1, 1, 32) * top * 8, rng.uniform(-1, 1, 32) * top * 8
    d[5, 0], d[6, 30] = top * 8, -np.nextafter(f32(top * 8), f32(np.inf))
    mid = [17, 19, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, -2.0 ** -11] if bits == 8 else \
        [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5, -0.2]
    d[7] = 0
    d[7, :len(mid)], d[7, 16:16 + len(mid)], d[7, 31] = mid, -np.asarray(mid), top
    d[8] = rng.standard_normal(32) * 1e-3
    d = d.reshape(1, -1)[:, :8 * 32 + 7]
    for R in (None, np.zeros_like(d)):
        row = check_encode(np.zeros(d.shape[1], f32), -d, R, bits, f"special {bits}")[0]
        assert list(row["scales"][:8]) == [0, 0, 27 - emax, 0, 0, 130, 131, 127]
        assert not row["codes"][:64].any() and not row["codes"][96:160].any()
        assert row["codes"][7 * 32 + len(mid) - 1] == 1 << (bits - 1)  # -0: the sign alone


def check_decode(pay, n, bits, master, mom, hp, first, K_out, tag, bf16=False, off=0):
    from gym_amd import ops
    S = pay.shape[0]
    buf, rb = payload_buf(S, n, bits, pay)
    PM, PB = Placed(master, off=off), Placed(mom, off=off)
    PD = Placed(np.full((max(K_out, 1), n), 3.5, f32), ld=(n + 7) // 8 * 8 + 8, off=off,
                dtype=torch.bfloat16 if bf16 else torch.float32)
    before = buf.clone()
    ops.diloco_outer_mx(buf, PM.view[:n], PB.view[:n] if hp["momentum"] else None, PD.rows if K_out else None, n, bits,
                        float(S), hp["lr"], hp["momentum"], hp["dampening"], hp["weight_decay"], hp["nesterov"], first)
    wm, wb, _ = M.decode_outer(pay, n, bits, float(S), master, None if first else mom, hp, first)
    assert same(PM.data(), wm) and PM.outside_untouched() and PB.outside_untouched(), (tag, "master")
    assert same(PB.data(), wb) if hp["momentum"] else PB.untouched(), (tag, "momentum")
    assert torch.equal(buf, before) and PD.outside_untouched(), tag
    if K_out:
        assert all(np.array_equal(r, to_dtype_bits(wm, bf16)) for r in PD.data_bits()), (tag, "dst")
    else:
        assert PD.untouched(), tag


@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("n", [33, 520, 4096 + 40])
@pytest.mark.parametrize("bits", [8, 4])
def test_decode_outer_step(bits, n, S):
    """First step with Nesterov momentum, a later step without momentum, weight decay on;
    bf16 rows; everything one element off alignment."""
    master, X, R = data(200 + n + S, S, n)
    pay = M.encode(master, X, R, bits)[0]
    mom = (np.random.default_rng(n).standard_normal(n) * 1e-3).astype(f32)
    for K_out in (0, 1, 3):
        check_decode(pay, n, bits, master, np.full(n, SENT, f32), HP, True, K_out, ("first", K_out))
        check_decode(pay, n, bits, master, mom, HP, False, K_out, ("later", K_out), bf16=K_out == 3)
    check_decode(pay, n, bits, master, mom, dict(HP, momentum=0.0, nesterov=False), False, 1, "plain")
    check_decode(pay, n, bits, master, mom, HP, False, 3, "offset", off=1)


@pytest.mark.parametrize("comp", ["mxfp8", "mxfp4"])
def test_engine_three_steps_with_feedback(comp):
    from gym_amd.comm import Collective
    from gym_amd.engine import MX_FORMATS, DiLoCoOuterMX
    K, n, bits = 3, 700, MX_FORMATS[comp]
    master, _, _ = data(5, K, n)
    eng = DiLoCoOuterMX(Collective(), K, n, DEV, torch.float32, bits=bits, error_feedback=True, **HP)
    eng.init_master(torch.from_numpy(master).to(DEV))
    reps, mom, resid = torch.full((K, n + 9), SENT, device=DEV), None, np.zeros((K, n), f32)
    for step in range(3):
        x = data(50 + step, K, n)[1] - data(50 + step, K, n)[0] + master
        reps[:, :n] = torch.from_numpy(x).to(DEV)
        x = reps[:, :n].cpu().numpy()
        pay, resid, _ = M.encode(master, x, resid, bits)
        master, mom, _ = M.decode_outer(pay, n, bits, K, master, mom, HP, step == 0)
        eng(reps)
        got = reps.cpu().numpy()
        assert np.array_equal(eng.payload.cpu().numpy(), pay) and same(eng.residual.cpu().numpy(), resid), step
        assert same(eng.master.cpu().numpy(), master) and same(eng.mom.cpu().numpy(), mom), step
        assert all(same(got[k, :n], master) for k in range(K)) and (got[:, n:] == SENT).all(), step


def test_replica_mode_mxfp4_nodes_agree_with_the_oracle():
    """Three nodes, H = 2, two outer events: every node holds the same bits, and they are
    the oracle's decode of the exchanged payload on the master and momentum before it."""
    import replica_scenarios as R
    from gym_amd.engine import DiLoCoOuterMX
    from gym_amd.replica import ReplicaRunner
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    dev = torch.device(DEV)
    torch.manual_seed(42)
    models = [R._model("x", dev) for _ in range(3)]
    s = DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), H=2, outer_compression="mxfp4",
                       outer_error_feedback=True)
    runner = ReplicaRunner(s, models, rank=0, num_nodes=3)
    eng, events = runner.outer, 0
    assert type(eng) is DiLoCoOuterMX and eng.bits == 4 and eng.residual is not None
    for t_ in range(5):
        m0, b0, first = eng.master.cpu().numpy(), eng.mom.cpu().numpy(), eng.first
        runner.zero_grad()
        for k, m in enumerate(models):
            R._set_grads(m, k, t_, dev)
        runner.step()
        if not np.array_equal(eng.master.cpu().numpy(), m0):
            events += 1
            want = M.decode_outer(eng.payload.cpu().numpy(), eng.n, 4, 3.0, m0, b0, eng.hp, first)[0]
            rows = runner.ra.flat_set.cpu().numpy()[:, :eng.n]
            assert all(same(rows[k], want) for k in range(3)) and eng.residual.cpu().numpy().any(), t_
    assert events == 2
