"""The streaming outer step on the MI355X: FragmentedOuter over DiLoCoOuterStream
against the numpy replay (tests/stream_checks.py), the replica runner's fragments
before and after a merge, a small Trainer.fit in both execution modes, and one
send / receive round over an asynchronous RCCL all-reduce."""
import functools
import os

import numpy as np
import pytest
import torch

import quant_checks as Q
import stream_checks as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
HP = dict(lr=0.7, momentum=0.9, nesterov=True, dampening=0.0, weight_decay=1e-3)
CUTS = [0, 1024, 1536, 2560]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gym_amd import _lib
    _lib.lib()


def _host(x):
    torch.cuda.synchronize()
    return x.detach().cpu().float().numpy()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.int32), np.ascontiguousarray(b, f32).view(np.int32))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_fragmented_outer_on_the_device_follows_the_replay(bf16):
    """K = 4 rows of ld > n, three fragments, H = 6, tau = 2, alpha = 0.5, three outer
    periods with the rows perturbed on every step: rows, master and momentum bit for bit
    after every step (bf16 rows: the staged sum is a bf16 row)."""
    from gym_amd.comm import Collective
    from gym_amd.engine import DiLoCoOuterStream, FragmentedOuter
    K, n, H, tau, alpha, steps = 4, CUTS[-1], 6, 2, 0.5, 19
    dtype = torch.bfloat16 if bf16 else torch.float32
    rng = np.random.default_rng(2)
    x0 = np.tile((rng.standard_normal(n) * 0.02).astype(f32), (K, 1))
    deltas = (rng.standard_normal((steps, K, n)) * (4e-3 if bf16 else 1e-3)).astype(f32)
    if bf16:
        x0, deltas = Q.bf16_round(x0), Q.bf16_round(deltas)
    want = S.run(x0, deltas, CUTS, H, tau, alpha, HP, bf16=bf16)
    engines = [DiLoCoOuterStream(Collective(), K, b - a, DEV, dtype, delay=tau, mix=alpha, **HP)
               for a, b in zip(CUTS, CUTS[1:])]
    fo = FragmentedOuter(engines, CUTS, H, tau)
    reps = torch.full((K, n + 24), -7.25, device=DEV, dtype=dtype)
    reps[:, :n] = torch.from_numpy(x0).to(DEV).to(dtype)
    fo.init_master(reps[0].float())
    d_dev = torch.from_numpy(deltas).to(DEV).to(dtype)
    merged = []
    for t in range(steps):
        reps[:, :n] += d_dev[t]
        fo.step(reps, t)
        w = want[t]
        got = _host(reps)
        assert _same(got[:, :n], w["rows"]), t
        assert _same(np.concatenate([_host(e.master) for e in engines]), w["master"]), t
        assert _same(np.concatenate([_host(e.mom) for e in engines]), w["mom"]), t
        assert (got[:, n:] == -7.25).all()
        lens = [CUTS[f + 1] - CUTS[f] for kind, f in w["events"] if kind == "merge"]
        assert fo.launch_elems == lens
        merged += [(t, f) for kind, f in w["events"] if kind == "merge"]
    assert merged == [(4, 2), (6, 1), (8, 0), (10, 2), (12, 1), (14, 0), (16, 2), (18, 1)]
    assert fo.due == [20, None, None] and not _same(got[0, :n], got[1, :n])
    kept = reps.clone()
    fo.finish()
    torch.cuda.synchronize()
    assert fo.due == [None] * 3 and torch.equal(reps, kept)


def test_one_fragment_no_delay_no_mix_equals_diloco_outer_on_the_device():
    from gym_amd.comm import Collective
    from gym_amd.engine import DiLoCoOuter, DiLoCoOuterStream, FragmentedOuter
    K, n, H, steps = 3, 2560 + 8, 4, 10  # outer steps at 4 and 8, one inner step after the last
    rng = np.random.default_rng(3)
    a = torch.from_numpy(np.tile((rng.standard_normal(n) * 0.02).astype(f32), (K, 1))).to(DEV)
    b = a.clone()
    deltas = torch.from_numpy((rng.standard_normal((steps, K, n)) * 1e-3).astype(f32)).to(DEV)
    fo = FragmentedOuter([DiLoCoOuterStream(Collective(), K, n, DEV, torch.float32, **HP)], [0, n], H, 0)
    ref = DiLoCoOuter(Collective(), K, n, DEV, torch.float32, placement=False, **HP)
    fo.init_master(a[0])
    ref.init_master(b[0])
    assert fo.engines[0].stage is None
    for t in range(steps):
        a += deltas[t]
        b += deltas[t]
        fo.step(a, t)
        if t % H == 0 and t > 0:
            ref(b)
            assert fo.launch_elems == [n] == ref.launch_elems
        assert torch.equal(a, b), t
    assert torch.equal(fo.engines[0].master, ref.master) and torch.equal(fo.engines[0].mom, ref.mom)
    assert not torch.equal(a[0], a[1]) and torch.isfinite(a).all()


@pytest.mark.parametrize("alpha", [0.5, 0.0])
def test_replica_runner_fragments_before_and_after_a_merge(alpha):
    """ReplicaRunner, 3 nodes, H = 4, F = 2, tau = 1: fragment 1 [2048, ld) sends at step
    2 and merges at step 3, fragment 0 [0, 2048) sends at 4 and merges at 5.  With
    alpha = 0.5 the nodes still differ inside a fragment after its merge but are closer
    than before it (every pairwise difference is halved); with alpha = 0 they are equal
    inside it.  The other fragment is not touched by that merge."""
    import replica_scenarios as R
    from gym_amd.engine import DiLoCoOuterStream, FragmentedOuter
    from gym_amd.replica import ReplicaRunner
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    dev = torch.device(DEV)
    torch.manual_seed(42)
    models = [R._model("x", dev) for _ in range(3)]
    s = DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), H=4, num_fragments=2, outer_delay=1,
                       outer_mix=alpha)
    runner = ReplicaRunner(s, models, rank=0, num_nodes=3)
    fo = runner.outer
    assert type(fo) is FragmentedOuter and all(type(e) is DiLoCoOuterStream for e in fo.engines)
    assert fo.bounds == [0, 2048, runner.ra.ld] and fo.delay == 1 and fo.H == 4
    seen = {}
    inner_step = fo.step

    def recording_step(P, local_step):
        before = _host(P).copy()
        inner_step(P, local_step)
        seen[local_step] = (before, _host(P).copy(), list(fo.launch_elems))

    fo.step = recording_step
    for t in range(6):
        runner.zero_grad()
        for k, m in enumerate(models):
            R._set_grads(m, k, t, dev)
        runner.step()
    runner.finish()

    def spread(rows):
        return max(float(np.abs(rows[i] - rows[j]).max()) for i in range(3) for j in range(i))

    for t, (lo, hi), (olo, ohi) in ((3, (2048, runner.ra.ld), (0, 2048)), (5, (0, 2048), (2048, runner.ra.ld))):
        before, after, launched = seen[t]
        assert launched == [hi - lo]
        assert np.isfinite(after).all()
        assert np.array_equal(before[:, olo:ohi], after[:, olo:ohi])  # the other fragment: untouched
        assert spread(before[:, olo:ohi]) > 0
        if alpha == 0:
            assert spread(after[:, lo:hi]) == 0 and spread(before[:, lo:hi]) > 0
        else:
            assert 0 < spread(after[:, lo:hi]) < spread(before[:, lo:hi])
            assert not np.array_equal(before[:, lo:hi], after[:, lo:hi])
    for t in (0, 1, 2, 4):  # no merge lands: a send leaves the rows as they are
        assert np.array_equal(seen[t][0], seen[t][1]) and seen[t][2] == []


def _fit(replicas, port, **kw):
    from tiny_models import TinyMLP, dataset
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    from gym_amd.trainer import LocalTrainer
    torch.manual_seed(0)
    tr = LocalTrainer(TinyMLP(), dataset(256), dataset(64, seed=1), start_port=port)
    strategy = DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), H=4, **kw)
    final = tr.fit(num_epochs=1, strategy=strategy, num_nodes=2, max_steps=10, devices=[0], batch_size=16,
                   minibatch_size=16, val_size=16, val_interval=100, replicas_per_process=replicas,
                   keep_node_states=True)
    return tr.node_states, final


@functools.lru_cache(maxsize=None)
def _plain_fit():
    """Plain DiLoCoStrategy, both nodes in one process: computed once, read by two tests."""
    return _fit(2, 22740)[0]


def _equal_states(a, b):
    assert len(a) == len(b) == 2
    for r in range(2):
        for name in a[r]:
            assert torch.equal(a[r][name], b[r][name]), (r, name)


def test_trainer_fit_two_replicas_equal_two_processes():
    """LocalTrainer.fit, TinyMLP, 2 nodes, H = 4, F = 2, tau = 1, alpha = 0.5, 10 steps:
    both nodes in one process (replicas_per_process=2) against one process per node over
    gloo on the one GPU.  The staged sum of two rows has one order, so every node's
    final parameters are bit-identical between the modes."""
    kw = dict(num_fragments=2, outer_delay=1, outer_mix=0.5)
    rep, final_rep = _fit(2, 22700, **kw)
    proc, final_proc = _fit(1, 22720, **kw)
    _equal_states(rep, proc)
    assert any(not torch.equal(rep[0][k], rep[1][k]) for k in rep[0])  # mixed: the nodes keep their own progress
    for a, b in zip(final_rep.parameters(), final_proc.parameters()):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    # ...and it is another run than plain DiLoCo's
    plain = _plain_fit()
    assert any(not torch.equal(rep[0][k], plain[0][k]) for k in rep[0])


def test_trainer_fit_with_the_options_at_their_defaults_is_plain_diloco():
    """F = 1, tau = 0, alpha = 0 spelled out: plain DiLoCoStrategy, bit for bit."""
    spelled, _ = _fit(2, 22760, num_fragments=1, outer_delay=0, outer_mix=0.0)
    _equal_states(spelled, _plain_fit())


def _rccl_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(torch.device(DEV))
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(DEV))
    try:
        from gym_amd.comm import Collective
        from gym_amd.engine import DiLoCoOuterStream
        coll = Collective(force_exchange=True)
        assert coll.rccl and coll.exchange and coll.world == 1
        data = np.load(os.path.join(out_dir, "in.npz"))
        K, n = data["x0"].shape
        eng = DiLoCoOuterStream(coll, K, n, DEV, torch.float32, delay=2, mix=0.5, **HP)
        reps = torch.full((K, n + 16), -7.25, device=DEV)
        reps[:, :n] = torch.from_numpy(data["x0"]).to(DEV)
        eng.init_master(reps[0])
        out = {}
        for r in range(2):
            eng.send(reps)
            assert eng._work is not None and hasattr(eng._work, "wait")
            reps[:, :n] += torch.from_numpy(data["deltas"][r]).to(DEV)  # inner steps under the exchange
            eng.receive(reps)
            torch.cuda.synchronize()
            out[f"rows{r}"] = reps.cpu().numpy().copy()
            out[f"master{r}"] = eng.master.cpu().numpy().copy()
            out[f"mom{r}"] = eng.mom.cpu().numpy().copy()
            assert eng._work is None and eng.launch_elems == [n] and eng.first is False
        np.savez(os.path.join(out_dir, "out.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_send_receive_over_an_async_rccl_all_reduce(tmp_path):
    """One DiLoCoOuterStream under a world-1 "nccl" group with the exchange forced: send
    starts all_reduce(async_op=True) on RCCL's stream, the rows move on, receive waits on
    the handle (ordering the current stream after the collective) and merges.  Two
    rounds against the oracle, bit for bit."""
    import torch.multiprocessing as mp
    from strategy_scenarios import free_port
    K, n = 3, 2560 + 8
    rng = np.random.default_rng(9)
    x0 = np.tile((rng.standard_normal(n) * 0.02).astype(f32), (K, 1))
    x0 = (x0 + rng.standard_normal((K, n)) * 1e-3).astype(f32)
    deltas = (rng.standard_normal((2, K, n)) * 1e-3).astype(f32)
    np.savez(tmp_path / "in.npz", x0=x0, deltas=deltas)
    mp.spawn(_rccl_worker, args=(1, free_port(), str(tmp_path)), nprocs=1, join=True)
    got = np.load(tmp_path / "out.npz")
    X, master, mom = x0.copy(), x0[0].copy(), None
    for r in range(2):
        stage = np.zeros(n, f32)
        for row in X:
            stage = stage + row
        X = (X + deltas[r]).astype(f32)
        master, mom, X = S.merge(stage[None, :], K, master, mom, HP, r == 0, 0.5, X, False)
        assert _same(got[f"rows{r}"][:, :n], X) and (got[f"rows{r}"][:, n:] == -7.25).all(), r
        assert _same(got[f"master{r}"], master) and _same(got[f"mom{r}"], mom), r
    assert not _same(X[0], X[1])
