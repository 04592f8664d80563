"""DiLoCoOuterQuant and the outer_compression options on the MI355X: the engine on a
crafted replica set against the numpy oracle (tests/quant_checks.py), a small
Trainer.fit in both execution modes, and the error-feedback invariant."""
import numpy as np
import pytest
import torch

import quant_checks as Q

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gym_amd import _lib
    _lib.lib()


def _host(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy()


def _same(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.int32), np.asarray(b, f32).view(np.int32))


@pytest.mark.parametrize("comp,feedback", [("int8", True), ("int4", True), ("int8", False), ("int4", False)])
def test_engine_on_a_crafted_set_follows_the_oracle(comp, feedback):
    """Four nodes in one process on a [4, ld] set (ld > n, the tail a sentinel), three
    outer steps with weight decay and Nesterov momentum: payload, residual, master,
    momentum and every row bit for bit, the state carried on the device."""
    from gym_amd.comm import Collective
    from gym_amd.engine import QUANT_BITS, DiLoCoOuterQuant
    K, n, ld = 4, 4096 + 256 + 87, 4096 + 256 + 87 + 9
    bits = QUANT_BITS[comp]
    hp = dict(lr=0.7, momentum=0.9, nesterov=True, dampening=0.0, weight_decay=1e-3)
    rng = np.random.default_rng(11)
    start = (rng.standard_normal(n) * 0.02).astype(f32)
    eng = DiLoCoOuterQuant(Collective(), K, n, DEV, torch.float32, bits=bits, error_feedback=feedback, **hp)
    eng.init_master(torch.from_numpy(start).to(DEV))
    assert eng.payload.shape == (K, Q.row_bytes(n, bits)) and eng.payload_bytes_per_node == Q.row_bytes(n, bits)
    reps = torch.full((K, ld), -7.25, device=DEV)
    master, mom = start, None
    resid = np.zeros((K, n), f32) if feedback else None
    for step in range(3):
        x = (master + rng.standard_normal((K, n)) * 1e-3).astype(f32)
        x[1, 256:512] = master[256:512]  # node 1 did not move in block 1: its scale is 0 on the first step
        reps[:, :n] = torch.from_numpy(x).to(DEV)
        pay, resid, _ = Q.encode(master, x, resid, bits)
        master, mom, g = Q.decode_outer(pay, n, bits, K, master, mom, hp, step == 0)
        eng(reps)
        assert np.array_equal(_host(eng.payload), pay), (step, "payload")
        assert _same(_host(eng.master), master) and _same(_host(eng.mom), mom), step
        if feedback:
            assert _same(_host(eng.residual), resid) and resid.any()
        got = _host(reps)
        assert all(_same(got[k, :n], master) for k in range(K)) and (got[:, n:] == -7.25).all()
        assert eng.launch_elems == [n] and eng.first is False and g.any()
    assert eng.placement["placed"] is False
    with pytest.raises(ValueError, match="no one-pass masked outer step"):
        eng(reps, sparse_mask=torch.zeros(70, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("comp", ["int8", "int4"])
def test_error_feedback_tracks_the_true_sum(comp):
    """Two nodes x 64 elements whose delta d is the same on every outer step (lr = 0
    keeps the master, the rows are put back), T = 40 steps with error feedback.  Per
    step and element d + R_{t-1} = deq_t + R_t up to fp32 rounding, so
        sum_t deq_t - T d = R_0 - R_T = -R_T,
    and |R_T| <= s_T / 2 with s_T = max|d + R_{T-1}| / qmax <= (D + s_{T-1} / 2) / qmax,
    D = max|d| over the block; s_0 = 0, so by induction s_t <= D / (qmax - 1/2) =: step.
    The fp32 roundings add at most 2 ulp(2 D) per step, T * 2^-21 D in all, far below
    step / 2 = D / 13 (int4) or D / 253 (int8).  So the running sum of dequantised
    gradients stays within one quantisation step of the running sum of true deltas;
    without feedback the error would grow as T times the per-step error."""
    from gym_amd.comm import Collective
    from gym_amd.engine import QUANT_BITS, DiLoCoOuterQuant
    K, n, T = 2, 64, 40
    bits, qmax = QUANT_BITS[comp], Q.QMAX[QUANT_BITS[comp]]
    master = np.linspace(-0.5, 0.5, n).astype(f32)
    d = np.stack([np.linspace(-1.0, 1.0, n) * 1e-3, np.cos(np.arange(n)) * 3e-3 + 1e-4]).astype(f32)
    x = (master - d).astype(f32)
    d = (master - x).astype(f32)  # the delta the kernel forms, exactly
    eng = DiLoCoOuterQuant(Collective(), K, n, DEV, torch.float32, bits=bits, error_feedback=True, lr=0.0,
                           momentum=0.0, nesterov=False)
    eng.init_master(torch.from_numpy(master).to(DEV))
    rows = torch.from_numpy(x).to(DEV)
    reps = torch.empty_like(rows)
    total = np.zeros((K, n), np.float64)
    worst_plain = 0.0
    step_size = np.abs(d).max(axis=1, keepdims=True).astype(np.float64) / (qmax - 0.5)
    for t_ in range(1, T + 1):
        reps.copy_(rows)
        eng(reps)
        assert _same(_host(eng.master), master)
        total += Q.dequant_rows(_host(eng.payload), n, bits).astype(np.float64)
        gap = np.abs(total - t_ * d.astype(np.float64))
        assert (gap <= step_size).all(), (t_, float((gap / step_size).max()))
        if t_ == 1:
            worst_plain = float((gap / step_size).max())
    print(f"{comp}: after {T} steps max gap {float((gap / step_size).max()):.4f} steps; one step alone {worst_plain:.4f}")
    # ...and what is still owed sits in the residual: R_T = -(sum_t deq_t - T d) up to those roundings
    owed = _host(eng.residual).astype(np.float64) + (total - T * d.astype(np.float64))
    assert (np.abs(owed) <= T * 2.0 ** -21 * np.abs(d).max()).all()


def test_replica_runner_nodes_agree_after_every_outer_step():
    """ReplicaRunner on the GPU, 3 nodes, H = 2: after each outer step every node holds
    the same bits (one decode wrote all rows); SPARTA+DiLoCo with compression runs the
    two modules in sequence."""
    import replica_scenarios as R
    from gym_amd.engine import DiLoCoOuterQuant
    from gym_amd.replica import ReplicaRunner
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec, SPARTADiLoCoStrategy
    dev = torch.device(DEV)
    inner = OptimSpec(torch.optim.AdamW, lr=1e-2)
    for make in (lambda: DiLoCoStrategy(optim_spec=inner, H=2, outer_compression="int4", outer_error_feedback=True),
                 lambda: SPARTADiLoCoStrategy(inner_optim=inner, H=2, p_sparta=0.1, outer_compression="int8")):
        torch.manual_seed(42)
        models = [R._model("x", dev) for _ in range(3)]
        s = make()
        runner = ReplicaRunner(s, models, rank=0, num_nodes=3)
        assert type(runner.outer) is DiLoCoOuterQuant and getattr(runner, "fuse", False) is False
        start = _host(runner.ra.flat_set[0]).copy()
        for t_ in range(5):
            runner.zero_grad()
            for k, m in enumerate(models):
                R._set_grads(m, k, t_, dev)
            runner.step()
            rows = _host(runner.ra.flat_set)
            if t_ % 2 == 0 and t_ > 0:
                assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], rows[2]), t_
                assert _same(rows[0], _host(runner.outer.master))
            elif isinstance(s, DiLoCoStrategy):
                assert not np.array_equal(rows[0], rows[1])
        assert not np.array_equal(rows[0], start) and np.isfinite(rows).all()
        if isinstance(s, SPARTADiLoCoStrategy):
            assert s.fuse_boundary is False and s.engine is runner.outer


def _fit(replicas, port):
    from tiny_models import TinyMLP, dataset
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    from gym_amd.trainer import LocalTrainer
    torch.manual_seed(0)
    tr = LocalTrainer(TinyMLP(), dataset(256), dataset(64, seed=1), start_port=port)
    strategy = DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), H=2, outer_compression="int8")
    final = tr.fit(num_epochs=1, strategy=strategy, num_nodes=2, max_steps=6, devices=[0], batch_size=16,
                   minibatch_size=16, val_size=16, val_interval=100, replicas_per_process=replicas,
                   keep_node_states=True)
    return tr.node_states, final


def test_trainer_fit_two_replicas_equal_two_processes():
    """LocalTrainer.fit, TinyMLP, 2 nodes, H = 2, 6 steps, int8: both nodes in one
    process (replicas_per_process=2) against one process per node over gloo on the one
    GPU.  Both decode the same payload bytes in node order, so every node's final
    parameters are bit-identical between the modes."""
    rep, final_rep = _fit(2, 22600)
    proc, final_proc = _fit(1, 22620)
    assert len(rep) == len(proc) == 2
    for r in range(2):
        for name in rep[r]:
            assert torch.equal(rep[r][name], proc[r][name]), (r, name)
    assert any(not torch.equal(rep[0][k], rep[1][k]) for k in rep[0])  # one inner step after the last outer step
    for a, b in zip(final_rep.parameters(), final_proc.parameters()):
        assert torch.equal(a, b) and torch.isfinite(a).all()
