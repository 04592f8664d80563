"""ga_rht_encode, ga_diloco_outer_rht, DiLoCoOuterRHT and outer_compression="rht-int8" on the
MI355X, every byte and bit against tests/rht_checks.py, no tolerance.  A block is 256
elements and one wavefront, a workgroup 16 blocks: the sizes are a single element, a short /
whole / whole + short block and two workgroups with a short last block.  Buffers are longer
than the kernel is told; the rest is a sentinel."""
import numpy as np
import pytest
import torch

import quant_checks as Q
import rht_checks as H
from quant_checks import bf16_round, to_dtype_bits
from sgd_kernel_checks import DEV, SENT, Placed

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = [1, 255, 256, 257, 4396]
HP = dict(lr=0.7, momentum=0.9, nesterov=True, dampening=0.0, weight_decay=1e-3)
VARIANTS = {"nesterov": HP, "dampening": dict(HP, nesterov=False, dampening=0.1, weight_decay=0.0),
            "plain": dict(HP, momentum=0.0, nesterov=False)}
PATHS = {"vector": {}, "offset": dict(off=1), "odd ld": dict(odd=1)}  # the last two: the element path


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def same(a, b):  # bit-identical fp32 arrays (NaNs: a NaN in the same places)
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan])


def data(seed, K, n):  # a heavy-tailed delta: 3% of the entries 100 times larger
    rng = np.random.default_rng(seed)
    master = (rng.standard_normal(n) * 0.02).astype(f32)
    X = (master + rng.standard_normal((K, n)) * 1e-3 * np.where(rng.random((K, n)) < 0.03, 100, 1)).astype(f32)
    return master, X, (rng.standard_normal((K, n)) * 2e-5).astype(f32)


def payload_buf(S, n, bits, rows=None):  # S rows of stride row_bytes + 32 in a 0xA5-filled allocation
    rb = Q.row_bytes(n, bits)
    buf = torch.full((S, rb + 32), 0xA5, dtype=torch.uint8, device=DEV)
    if rows is not None:
        buf[:, :rb] = torch.from_numpy(rows).to(DEV)
    return buf, rb


def check_encode(master, X, R, bits, seed, tag, off=0, odd=0, bf16=False):
    """The encode against the oracle; returns the oracle's (payload, residual, row dicts)."""
    from gym_amd import ops
    K, n = X.shape
    ld = (n + 3) // 4 * 4 + 4 + odd
    PX = Placed(X, ld=ld, off=off, dtype=torch.bfloat16 if bf16 else torch.float32)
    PM, PR = Placed(master, off=off), Placed(R, ld=ld, off=off) if R is not None else None
    buf, rb = payload_buf(K, n, bits)
    ops.rht_encode(PX.rows, PM.view[:n], PR.rows if PR else None, buf, n, bits, seed)
    want = H.encode(master, X, R, bits, seed)
    got = buf.cpu().numpy()
    bad = np.flatnonzero((got[:, :rb] != want[0]).reshape(-1))
    assert bad.size == 0, (tag, "payload", bad[:8], got[:, :rb].reshape(-1)[bad[:8]], want[0].reshape(-1)[bad[:8]])
    assert (got[:, rb:] == 0xA5).all() and PX.untouched() and PM.untouched(), tag
    assert R is None or (same(PR.data(), want[1]) and PR.outside_untouched()), (tag, "residual")
    return want


def check_decode(pay, n, bits, seed, master, mom, hp, first, K_out, tag, bf16=False, off=0, odd=0):
    """The decode + outer step against the oracle; returns the oracle's (master, momentum)."""
    from gym_amd import ops
    S = pay.shape[0]
    buf, rb = payload_buf(S, n, bits, pay)
    PM, PB = Placed(master, off=off), Placed(mom, off=off)
    PD = Placed(np.full((max(K_out, 1), n), 3.5, f32), ld=(n + 3) // 4 * 4 + 4 + odd, off=off,
                dtype=torch.bfloat16 if bf16 else torch.float32)
    before = buf.clone()
    ops.diloco_outer_rht(buf, PM.view[:n], PB.view[:n] if hp["momentum"] else None, PD.rows if K_out else None, n,
                         bits, float(S), hp["lr"], hp["momentum"], hp["dampening"], hp["weight_decay"], hp["nesterov"],
                         first, seed)
    wm, wb, _ = H.decode_outer(pay, n, bits, float(S), master, None if first else mom, hp, first, seed)
    assert same(PM.data(), wm) and PM.outside_untouched() and PB.outside_untouched(), (tag, "master")
    assert same(PB.data(), wb) if hp["momentum"] else PB.untouched(), (tag, "momentum")
    assert torch.equal(buf, before) and PD.outside_untouched(), tag
    if K_out:
        assert all(np.array_equal(r, to_dtype_bits(wm, bf16)) for r in PD.data_bits()), (tag, "dst")
    else:
        assert PD.untouched(), tag
    return wm, wb


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", [8, 4])
def test_encode_bytes_and_residual(bits, n, feedback, bf16):
    """Two seeds; at the largest size also the element path (an offset base, an odd ld)."""
    for K, seed in ((1, 0), (3, 77)):
        master, X, R = data(100 + n + K, K, n)
        for path in (PATHS if n == SIZES[-1] else ["vector"]):
            check_encode(master, bf16_round(X) if bf16 else X, R if feedback else None, bits, seed, (K, seed, path),
                         bf16=bf16, **PATHS[path])
    # a single element's codes depend on its own sign alone, which the two seeds may share
    assert n == 1 or not np.array_equal(H.encode(master, X, None, bits, 0)[0], H.encode(master, X, None, bits, 77)[0])


@pytest.mark.parametrize("bits", [8, 4])
def test_encode_special_blocks(bits):
    """Blocks built by hand (master = 0 and x = -d, so d is exact): all zero; a single
    entry A (every rotated value is +-A / 16, every q = +-qmax); a single entry that puts
    amax just below and at 2^-100; a NaN and an Inf element; identical values; a short
    tail.  The residual of a dead block is its delta."""
    qmax, tiny, rng = Q.QMAX[bits], f32(2.0 ** -100), np.random.default_rng(bits)
    d = np.zeros((8, 256), f32)
    d[1, 37], d[2, 5], d[3, 255] = 3.0, 16 * np.nextafter(tiny, f32(0)), -16 * tiny
    d[4], d[5] = rng.standard_normal(256), rng.standard_normal(256)
    d[4, 7], d[5, 9] = np.nan, -np.inf
    d[6], d[7] = 0.375, rng.standard_normal(256) * 1e-3
    d = d.reshape(1, -1)[:, :7 * 256 + 9]
    for R in (None, np.zeros_like(d)):
        _, resid, rows = check_encode(np.zeros(d.shape[1], f32), -d, R, bits, 5, f"special {bits}")
        s, q = rows[0]["scales"], rows[0]["q"]
        assert list(s[[0, 2, 4, 5]]) == [0, 0, 0, 0] and not q[[0, 2, 4, 5]].any() and q[6].any() and q[7].any()
        assert (np.abs(rows[0]["y"][1]) == f32(3.0 / 16)).all() and (np.abs(q[[1, 3]]) == qmax).all()
        assert s[1] == f32(3.0 / 16) / f32(qmax) and s[3] == tiny / f32(qmax)
        assert R is None or (same(resid[0, :256], d[0, :256]) and same(resid[0, 1024:1536], d[0, 1024:1536]))


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", [8, 4])
def test_decode_outer_step(bits, n, S):
    """First step with Nesterov momentum and a later step, weight decay on; fp32 and bf16
    rows; one element off alignment and an odd ld (the element path)."""
    seed = 77 if S == 3 else 0
    master, X, R = data(200 + n + S, S, n)
    pay = H.encode(master, X, R, bits, seed)[0]
    mom = (np.random.default_rng(n).standard_normal(n) * 1e-3).astype(f32)
    for K_out in (0, 1, 3):
        check_decode(pay, n, bits, seed, master, np.full(n, SENT, f32), HP, True, K_out, ("first", K_out))
        check_decode(pay, n, bits, seed, master, mom, HP, False, K_out, ("later", K_out), bf16=K_out == 3)
    check_decode(pay, n, bits, seed, master, mom, HP, False, 3, "offset", off=1, bf16=True)
    check_decode(pay, n, bits, seed, master, mom, HP, False, 3, "odd ld", odd=1)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("bits", [8, 4])
def test_three_step_chain_carries_master_momentum_and_residual(bits, variant):
    """K = S = K_out = 3 over two workgroups, three encode + decode pairs; the state the
    next pair starts from is the oracle's, which the device's was just found equal to.
    Every step's residual is the delta less what a decode of that row alone (divisor 1,
    lr 1, zero master: the oracle's, which check_decode holds the kernel to) takes off."""
    hp, K, n, seed = VARIANTS[variant], 3, 4396, 3
    one = dict(lr=1.0, momentum=0.0, nesterov=False, dampening=0.0, weight_decay=0.0)
    master, _, resid = data(31, K, n)
    mom = None
    for step in range(3):
        X = (master + data(40 + step, K, n)[1] - data(40 + step, K, n)[0]).astype(f32)
        pay, resid, rows = check_encode(master, X, resid, bits, seed, (variant, step))
        taken = -H.decode_outer(pay[:1], n, bits, 1.0, np.zeros(n, f32), None, one, True, seed)[0]
        assert same(resid[0], rows[0]["d"] - taken) and np.abs(resid[0]).max() < np.abs(rows[0]["d"]).max()
        master, mom = check_decode(pay, n, bits, seed, master, np.full(n, SENT, f32) if mom is None else mom, hp,
                                   step == 0, 3, (variant, step))


@pytest.mark.parametrize("comp", ["rht-int8", "rht-int4"])
def test_engine_three_steps_with_feedback(comp):
    from gym_amd.comm import Collective
    from gym_amd.engine import RHT_FORMATS, DiLoCoOuterRHT
    K, n, bits, seed = 3, 700, RHT_FORMATS[comp], 11
    master, _, _ = data(5, K, n)
    eng = DiLoCoOuterRHT(Collective(), K, n, DEV, torch.float32, bits=bits, error_feedback=True, seed=seed, **HP)
    eng.init_master(torch.from_numpy(master).to(DEV))
    reps, mom, resid = torch.full((K, n + 9), SENT, device=DEV), None, np.zeros((K, n), f32)
    for step in range(3):
        reps[:, :n] = torch.from_numpy(data(50 + step, K, n)[1] - data(50 + step, K, n)[0] + master).to(DEV)
        pay, resid, _ = H.encode(master, reps[:, :n].cpu().numpy(), resid, bits, seed)
        master, mom, _ = H.decode_outer(pay, n, bits, K, master, mom, HP, step == 0, seed)
        eng(reps)
        got = reps.cpu().numpy()
        assert np.array_equal(eng.payload.cpu().numpy(), pay) and same(eng.residual.cpu().numpy(), resid), step
        assert same(eng.master.cpu().numpy(), master) and same(eng.mom.cpu().numpy(), mom), step
        assert all(same(got[k, :n], master) for k in range(K)) and (got[:, n:] == SENT).all(), step


def _fit(replicas, port):
    from tiny_models import TinyMLP, dataset
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    from gym_amd.trainer import LocalTrainer
    torch.manual_seed(0)
    tr = LocalTrainer(TinyMLP(), dataset(256), dataset(64, seed=1), start_port=port)
    strategy = DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), H=2, outer_compression="rht-int8",
                              outer_error_feedback=True, outer_rotation_seed=4)
    tr.fit(num_epochs=1, strategy=strategy, num_nodes=2, max_steps=6, devices=[0], batch_size=16, minibatch_size=16,
           val_size=16, val_interval=100, replicas_per_process=replicas, keep_node_states=True)
    return tr.node_states


def test_trainer_fit_two_replicas_equal_two_processes():
    """LocalTrainer.fit, TinyMLP, 2 nodes, H = 2, 6 steps, rht-int8 with feedback: both nodes
    in one process against one process per node over gloo on the one GPU.  Both decode the
    same payload bytes in node order, so every node's final parameters are bit-identical."""
    rep, proc = _fit(2, 22800), _fit(1, 22820)
    assert len(rep) == len(proc) == 2
    assert all(torch.equal(rep[r][k], proc[r][k]) and torch.isfinite(rep[r][k]).all() for r in range(2) for k in rep[r])
