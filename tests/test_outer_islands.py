"""Island DiLoCo without a GPU: the options and what they refuse, the config, the draw
against FedAvg's, engine.DiLoCoOuterIslands against the numpy replay
(tests/island_checks.py), four nodes in one process against four gloo processes and
against 2 processes x 2 replicas, one island against DiLoCoStrategy, and the untouched
default paths of DiLoCo and FedAvg -- over the stand-ins of tests/fake_island_ops.py.
The kernel's arithmetic: test_gpu_outer_islands_kernel.py."""
import os
import pickle
import random

import numpy as np
import pytest
import torch

import island_checks as I
import replica_scenarios as R
import stream_checks as S

f32 = np.float32
HP = dict(lr=0.7, momentum=0.9, nesterov=True, dampening=0.0, weight_decay=1e-3)
NOMOM = dict(lr=0.5, momentum=0.0, nesterov=False, dampening=0.0, weight_decay=0.0)
SEED = 321


@pytest.fixture
def fake(monkeypatch):
    """The gym_amd modules pointed at fake_island_ops for one test, one fresh CALLS list."""
    import fake_island_ops as fi
    import fake_quant_ops as fq
    import fake_stream_ops as fs
    import gym_amd.engine as engine
    import gym_amd.fused_optim as fused_optim
    import gym_amd.replica as replica
    import gym_amd.strategy.diloco as diloco
    import gym_amd.strategy.federated_averaging as fedavg
    import gym_amd.strategy.strategy as strategy
    for mod in (engine, diloco, fedavg, fused_optim, replica):
        monkeypatch.setattr(mod, "ops", fi)
    monkeypatch.setattr(strategy, "require_gpu", lambda device: None)
    calls = []
    for mod in (fq, fs, fi):
        monkeypatch.setattr(mod, "CALLS", calls)
    return fi


class Local:
    world, rank, exchange, rccl, backend = 1, 0, False, False, "none"


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, f32)).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _strategy(**kw):
    from gym_amd.strategy import IslandDiLoCoStrategy, OptimSpec
    kw.setdefault("H", 2)
    return IslandDiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), **kw)


def _params(model):
    return [p.detach().float().numpy().copy() for p in model.parameters()]


# ------------------------------------------------------------------ options --
def test_options_are_validated_at_construction_and_at_node_init(fake):
    from gym_amd.strategy import DiLoCoStrategy, IslandDiLoCoStrategy, OptimSpec, SPARTADiLoCoStrategy
    for kw in (dict(outer_compression="int8"), dict(outer_compression="int4"), dict(outer_error_feedback=True),
               dict(num_fragments=2), dict(outer_delay=1), dict(outer_mix=0.5), dict(num_fragments=0)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            IslandDiLoCoStrategy(H=4, **kw)
    for bad in (0, -1, 2.0, "2", True):
        with pytest.raises(ValueError, match="island_size"):
            IslandDiLoCoStrategy(island_size=bad)
    for bad in (0, -2, 1.5, None, True):
        with pytest.raises(ValueError, match="H="):
            IslandDiLoCoStrategy(H=bad)
    for spec in (OptimSpec(torch.optim.Adam, lr=0.05), OptimSpec(torch.optim.AdamW), "adam",
                 OptimSpec(torch.optim.RMSprop, lr=0.1), OptimSpec(torch.optim.SGD, lr=0.1, maximize=True)):
        with pytest.raises(ValueError, match="plain torch.optim.SGD"):
            IslandDiLoCoStrategy(outer_optim_spec=spec)
    with pytest.raises(ValueError, match="Nesterov"):
        IslandDiLoCoStrategy(outer_optim_spec=OptimSpec(torch.optim.SGD, lr=0.1, nesterov=True))
    # the defaults spelled out are accepted; the siblings keep their options
    s = IslandDiLoCoStrategy(outer_compression=None, outer_error_feedback=False, num_fragments=1, outer_delay=0,
                             outer_mix=0.0)
    assert s.island_size == 2 and s.H == 100 and s.engine is None
    assert s.outer_optim_spec.cls is torch.optim.SGD and s.outer_optim_spec.kwargs == dict(lr=0.7, nesterov=True,
                                                                                           momentum=0.9)
    assert IslandDiLoCoStrategy(island_size=None).island_size is None
    DiLoCoStrategy(H=6, num_fragments=3, outer_delay=2, outer_mix=0.5)
    SPARTADiLoCoStrategy(H=4, outer_compression="int8")
    assert not isinstance(s, DiLoCoStrategy)
    # set after construction: node init refuses, in both modes, before any launch
    from gym_amd.replica import ReplicaRunner
    dev = torch.device("cpu")
    for attr, val, match in (("kwargs", dict(outer_delay=1), "outer_delay"), ("island_size", 0, "island_size"),
                             ("outer_optim_spec", OptimSpec(torch.optim.Adam, lr=0.05), "plain torch.optim.SGD"),
                             ("kwargs", dict(outer_compression="int8"), "outer_compression"), ("H", 0, "H=")):
        s = _strategy()
        setattr(s, attr, val)
        with pytest.raises(ValueError, match=match):
            s._init_node(R._model("x", dev), 0, 1)
        s = _strategy()
        setattr(s, attr, val)
        with pytest.raises(ValueError, match=match):
            ReplicaRunner(s, [R._model("x", dev) for _ in range(2)], rank=0, num_nodes=2)
    assert fake.CALLS == []


def test_config_pickle_and_exports(fake):
    import exogym.strategy as es
    import gym_amd.strategy as gs
    from gym_amd.replica import ReplicaRunner, replica_layout
    for name in ("IslandDiLoCoStrategy", "IslandDiLoCoCommunicator"):
        assert name in gs.__all__ and name in es.__all__ and getattr(es, name) is getattr(gs, name)
    import exogym.strategy.island_diloco as alias
    import gym_amd.strategy.island_diloco as impl
    assert alias is impl
    s = _strategy(H=7, island_size=3, max_norm=0.5, lr_scheduler="lambda_cosine", lr_scheduler_kwargs={})
    cfg = s.__config__()
    assert cfg["strategy"] == "IslandDiLoCoStrategy" and cfg["island_size"] == 3 and cfg["H"] == 7
    assert cfg["max_norm"] == 0.5 and cfg["placement"]["records"] == {} and "engine" not in cfg
    t = pickle.loads(pickle.dumps(s))  # strategies cross mp.spawn by pickle before _init_node
    assert type(t) is type(s) and t.H == 7 and t.island_size == 3 and t.max_norm == 0.5
    assert t.communication_modules[0].strategy is t and t.__config__() == cfg
    assert ReplicaRunner.supports(s) and replica_layout(4, ["cuda:0"], None, s) == (1, 4)
    # after node init the engine and its record are there
    t._init_node(R._model("x", torch.device("cpu")), 0, 1)
    from gym_amd.engine import DiLoCoOuterIslands
    assert type(t.engine) is DiLoCoOuterIslands and t.engine.K_local == 1 and t.engine.master.shape == (1, t.arena.n)
    rec = t.placement_records()["engine"]
    assert rec["placed"] is False and "no search" in rec["why"]
    assert t.__config__()["placement"]["records"]["engine"] == rec


# ----------------------------------------------------------------- the draw --
def _replica_run(K, steps, hook=None, seed=SEED, strategy=None, **kw):
    from gym_amd.replica import ReplicaRunner
    torch.manual_seed(42)
    random.seed(seed)
    dev = torch.device("cpu")
    models = [R._model("x", dev) for _ in range(K)]
    s = strategy or _strategy(**kw)
    runner = ReplicaRunner(s, models, rank=0, num_nodes=K)
    for t in range(steps):
        runner.zero_grad()
        for k, m in enumerate(models):
            R._set_grads(m, k, t, dev)
        runner.step()
        if hook is not None:
            hook(t, runner)
    return [_params(m) for m in models], s, runner


def _expected_draws(K, size, rounds, seed=SEED):
    random.seed(seed)
    return [I.draw(K, size) for _ in range(rounds)]


def test_the_draw_is_fedavgs(fake, monkeypatch):
    """Replica mode: under one random.seed the islands of three rounds are those
    FedAvgStrategy(island_size=s) averages (its row tables) and those of the
    independent statement in island_checks.draw."""
    from gym_amd.strategy import FedAvgStrategy, OptimSpec
    for K, size in ((5, 2), (4, 2), (7, 3)):
        del fake.CALLS[:]
        _replica_run(K, 7, island_size=size)
        got = [c[3] for c in fake.CALLS if c[0] == "islands"]
        want = _expected_draws(K, size, 3)
        assert got == want and len(got) == 3
        assert all(sorted(m for isl in rnd for m in isl) == list(range(K)) for rnd in got)
        assert [len(isl) for isl in got[0]] == [size] * (K // size) + ([K % size] if K % size else [])
        # FedAvg's runner, same seed: the rows it averages (one table launch per island with a local member)
        tables = []
        orig = fake.replica_mean

        def rec(src, dst, n=None, divisor=None, rows=None):
            if rows is not None:
                tables.append([int(r) for r in rows.tolist()])
            return orig(src, dst, n=n, divisor=divisor, rows=rows)

        monkeypatch.setattr(fake, "replica_mean", rec)
        fed = FedAvgStrategy(inner_optim=OptimSpec(torch.optim.SGD, lr=0.05), island_size=size, H=2)
        _replica_run(K, 7, strategy=fed)
        monkeypatch.setattr(fake, "replica_mean", orig)
        assert tables == [isl for rnd in want for isl in rnd]
    assert len({tuple(map(tuple, rnd)) for rnd in _expected_draws(7, 3, 3)}) > 1  # the islands change between rounds


# ---------------------------------------------- the engine against run() --
@pytest.mark.parametrize("hp", [HP, NOMOM], ids=["nesterov", "nomom"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_engine_follows_the_replay(fake, hp, dtype):
    """K = 5 in place, H = 2, 9 steps with the rows perturbed on every step, four rounds
    whose islands change: a short last island, an island of one, one island of all."""
    from gym_amd.engine import DiLoCoOuterIslands
    K, n, H, steps = 5, 777, 2, 9
    rounds = {2: [[1, 4], [0, 2], [3]], 4: [[0, 1, 2], [3, 4]], 6: [[2], [0, 1, 3, 4]], 8: [[0, 1, 2, 3, 4]]}
    bf16 = dtype == torch.bfloat16
    rng = np.random.default_rng(4)
    x0 = np.tile((rng.standard_normal(n) * 0.02).astype(f32), (K, 1))
    deltas = (rng.standard_normal((steps, K, n)) * (1e-2 if bf16 else 1e-3)).astype(f32)
    want = I.run(x0, deltas, H, rounds, hp, bf16=bf16)
    eng = DiLoCoOuterIslands(Local(), K, n, "cpu", dtype, **hp)
    assert eng.master.shape == (K, n) and eng.master.dtype == torch.float32
    assert (eng.mom is None) == (hp["momentum"] == 0) and eng.placement["placed"] is False
    reps = torch.full((K, n + 12), -7.25, dtype=dtype)
    reps[:, :n] = torch.from_numpy(x0).to(dtype)
    eng.init_master(reps[0])
    assert eng.first and all(torch.equal(eng.master[k], reps[0, :n].float()) for k in range(K))
    for t in range(steps):
        reps[:, :n] = (reps[:, :n].float() + torch.from_numpy(deltas[t])).to(dtype)
        before = len(fake.CALLS)
        if t in rounds:
            eng(reps, rounds[t], rounds[t], reps)
            assert fake.CALLS[before:] == [("islands", K, n, rounds[t], rounds[t], K, True)]  # ONE launch, in place
            assert eng.launch_elems == [n] and not eng.first
        w = want[t]
        assert _same(reps[:, :n].float().numpy(), w["rows"]), t
        assert _same(eng.master.numpy(), w["master"]), t
        if eng.mom is not None:
            assert _same(eng.mom.numpy(), w["mom"]), t
        assert (reps[:, n:].float() == -7.25).all()
    rows = want[2]["rows"]  # after the first round: partners bit-equal, islands different
    assert _same(rows[1], rows[4]) and _same(rows[0], rows[2]) and not _same(rows[1], rows[0])
    assert not _same(rows[3], rows[0]) and not _same(rows[3], rows[1])
    assert not _same(want[4]["rows"][3], want[4]["rows"][4])  # later partners differ: their masters do
    # only the islands with a local member are launched; none at all is an error
    before = len(fake.CALLS)
    one = DiLoCoOuterIslands(Local(), 1, n, "cpu", dtype, **hp)
    one.init_master(reps[0])
    own = reps[1:2].clone()
    one(reps, [[0, 3], [1, 2, 4]], [[-1, -1], [0, -1, -1]], own)
    assert fake.CALLS[before:] == [("islands", K, n, [[1, 2, 4]], [[0, -1, -1]], 1, False)]
    with pytest.raises(ValueError, match="no island has a local member"):
        one(reps, [[0, 3]], [[-1, -1]], own)


def test_the_oracle_is_pinned_to_the_merge_oracle():
    """One island, every member local: island_checks.step is stream_checks.merge at
    alpha = 0 (itself pinned to ga_diloco_outer) once per member, bit for bit."""
    rng = np.random.default_rng(8)
    K, n = 4, 515
    for hp, first, bf16 in ((HP, False, False), (HP, True, True), (NOMOM, False, True),
                            (dict(HP, nesterov=False, dampening=0.1), False, False)):
        master = (rng.standard_normal((K, n)) * 0.02).astype(f32)
        mom = (rng.standard_normal((K, n)) * 1e-3).astype(f32)
        src = (master[0] + rng.standard_normal((K, n)) * 1e-3).astype(f32)
        if bf16:
            src = I.bf16_round(src)
        has_mom = hp["momentum"] != 0
        gm, gb, gx = I.step(src, [list(range(K))], [list(range(K))], master, mom if has_mom else None, hp, first, bf16)
        for k in range(K):
            wm, wb, wx = S.merge(src, float(K), master[k], None if (first or not has_mom) else mom[k], hp, first, 0.0,
                                 src[k:k + 1], bf16)
            assert _same(gm[k], wm) and _same(gx[k], wx[0])
            if has_mom:
                assert _same(gb[k], wb)
    # a member with slot -1 is summed and not updated; unnamed state rows stay
    gm, gb, gx = I.step(src, [[0, 2]], [[-1, 1]], master, mom, HP, False, False)
    wm, wb, _ = S.merge(src[[0, 2]], 2.0, master[1], mom[1], HP, False, 0.0, None, False)
    assert sorted(gx) == [1] and _same(gm[1], wm) and _same(gb[1], wb)
    assert _same(gm[[0, 2, 3]], master[[0, 2, 3]]) and _same(gb[[0, 2, 3]], mom[[0, 2, 3]])


# ------------------------------ 4 nodes: one process, 4 processes, 2 x 2 --
GLOO_STEPS = 7
ISL_KW = dict(H=2, island_size=2, max_norm=1.0)


def _init_gloo(rank, world, port):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    import fake_island_ops
    fake_island_ops.install()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return fake_island_ops


def _process_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    fake = _init_gloo(rank, world, port)
    try:
        from gym_amd.engine import DiLoCoOuterIslands
        from gym_amd.strategy import FedAvgStrategy, OptimSpec
        from gym_amd.strategy.federated_averaging import AveragingCommunicator
        torch.manual_seed(42)
        random.seed(SEED)  # rank 0's draw
        dev = torch.device("cpu")
        model = R._model("x", dev)
        s = _strategy(**ISL_KW)
        s._init_node(model, rank, world)
        assert type(s.engine) is DiLoCoOuterIslands and s.engine.K_local == 1
        rows = []
        for t in range(GLOO_STEPS):
            s.zero_grad()
            R._set_grads(model, rank, t, dev)
            s.step()
            rows.append(s.arena.flat[:s.arena.n].numpy().copy())
        s.finish()
        calls = [c for c in fake.CALLS if c[0] == "islands"]
        assert len(calls) == 3 and len(fake.CALLS) == 3  # one launch per round and nothing else
        # over the island's sub-communicator: 2 gathered rows, this node's slot at its place
        assert all(c[1] == 2 and c[3] == [[0, 1]] and sorted(c[4][0]) == [-1, 0] and c[5] == 1 and not c[6]
                   for c in calls)
        mine = [c[4][0].index(0) for c in calls]
        # FedAvg's own draw under the same seed, and the launches its island path makes (unchanged)
        random.seed(SEED)
        comm = AveragingCommunicator(island_size=2)
        partners = [sorted(comm._select_partners(rank, world)) for _ in range(3)]
        means = []
        orig = fake.replica_mean

        def rec(src, dst, n=None, divisor=None, rows=None):
            means.append((src.shape[0], None if rows is None else rows.tolist()))
            return orig(src, dst, n=n, divisor=divisor, rows=rows)

        import gym_amd.strategy.federated_averaging as fedavg_mod
        fedavg_mod.ops = type("Ops", (), {"replica_mean": staticmethod(rec)})
        fed = FedAvgStrategy(inner_optim=OptimSpec(torch.optim.SGD, lr=0.05), island_size=2, H=2)
        m2 = R._model("x", dev)
        fed._init_node(m2, rank, world)
        for t in range(5):
            fed.zero_grad()
            R._set_grads(m2, rank, t, dev)
            fed.step()
        assert means == [(2, None)] * 2  # the gathered pair, every row a member: FedAvg's launches as before
        np.savez(os.path.join(out_dir, f"proc{rank}.npz"), rows=np.stack(rows), master=s.engine.master[0].numpy(),
                 mom=s.engine.mom[0].numpy(), partners=np.array(partners), mine=np.array(mine),
                 **{f"p{i}": p for i, p in enumerate(_params(model))})
    finally:
        dist.destroy_process_group()


def _replica_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    fake = _init_gloo(rank, world, port)
    try:
        from gym_amd.replica import ReplicaRunner
        K = 4 // world
        torch.manual_seed(42)
        random.seed(SEED)  # the first process's draw
        dev = torch.device("cpu")
        models = [R._model("x", dev) for _ in range(K)]
        s = _strategy(**ISL_KW)
        runner = ReplicaRunner(s, models, rank=rank, num_nodes=4)
        rows = []
        for t in range(GLOO_STEPS):
            runner.zero_grad()
            for k, m in enumerate(models):
                R._set_grads(m, rank * K + k, t, dev)
            runner.step()
            rows.append(runner.ra.flat_set.numpy().copy())
        calls = [c for c in fake.CALLS if c[0] == "islands"]
        assert len(calls) == 3 and len(fake.CALLS) == 3  # ONE launch per round for both local nodes
        assert all(c[1] == 4 and c[5] == K and not c[6] for c in calls)  # off the gathered set, not in place
        np.savez(os.path.join(out_dir, f"rep{rank}.npz"), rows=np.stack(rows), master=runner.outer.master.numpy(),
                 mom=runner.outer.mom.numpy())
    finally:
        dist.destroy_process_group()


def test_four_nodes_in_one_process_equal_four_processes_and_two_by_two(tmp_path, fake):
    """IslandDiLoCoStrategy(H=2, island_size=2, max_norm=1) over 7 steps, three rounds:
    every node's parameters on every step, its master and its momentum are bit-identical
    between 4 replicas in one process, 4 gloo processes and 2 gloo processes x 2
    replicas -- the island's ascending-node sum has one order however the nodes are split."""
    import torch.multiprocessing as mp
    from strategy_scenarios import free_port
    mp.spawn(_process_worker, args=(4, free_port(), str(tmp_path)), nprocs=4, join=True)
    mp.spawn(_replica_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    proc = [dict(np.load(tmp_path / f"proc{r}.npz")) for r in range(4)]
    rep = [dict(np.load(tmp_path / f"rep{r}.npz")) for r in range(2)]
    rows = []
    nodes, s, runner = _replica_run(4, GLOO_STEPS, hook=lambda t, r: rows.append(r.ra.flat_set.numpy().copy()),
                                    **ISL_KW)
    n = proc[0]["rows"].shape[1]
    draws = _expected_draws(4, 2, 3)
    calls = [c for c in fake.CALLS if c[0] == "islands"]
    assert calls == [("islands", 4, runner.ra.ld, d, d, 4, True) for d in draws] == fake.CALLS  # in place
    assert runner.outer.launch_elems == [runner.ra.ld] and s.engine is runner.outer
    for r in range(4):
        for t in range(GLOO_STEPS):
            assert _same(proc[r]["rows"][t], rows[t][r, :n]), ("process", r, t)
            assert _same(rep[r // 2]["rows"][t][r % 2], rows[t][r]), ("2x2", r, t)
        for i, p in enumerate(nodes[r]):
            assert _same(proc[r][f"p{i}"], p), (r, i)
        assert _same(proc[r]["master"], runner.outer.master[r, :n].numpy())
        assert _same(proc[r]["mom"], runner.outer.mom[r, :n].numpy())
        assert _same(rep[r // 2]["master"][r % 2], runner.outer.master[r].numpy())
        assert _same(rep[r // 2]["mom"][r % 2], runner.outer.mom[r].numpy())
        # the process-mode draw is FedAvg's: the partners its communicator selects under the same seed
        want = [next(isl for isl in d if r in isl) for d in draws]
        assert [list(p) for p in proc[r]["partners"]] == want
        assert list(proc[r]["mine"]) == [isl.index(r) for isl in want]
    # after the first round (step 2): partners bit-equal, the islands different; later partners differ
    a, b = draws[0]
    first = rows[2]
    assert _same(first[a[0]], first[a[1]]) and _same(first[b[0]], first[b[1]]) and not _same(first[a[0]], first[b[0]])
    assert draws[1] != draws[0] or draws[2] != draws[0]
    last = rows[GLOO_STEPS - 1]
    assert np.isfinite(last).all() and not _same(last[draws[2][0][0]], last[draws[2][0][1]])


# ------------------------------------------------- one island is DiLoCo --
def test_one_island_is_diloco(fake):
    """island_size=None (and >= num_nodes) in one process: one island of all nodes and no
    draw, every node's master stays the same, so rows and master are DiLoCoStrategy's bit
    for bit on every step."""
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    K, steps = 3, 7
    sgd = OptimSpec(torch.optim.SGD, lr=0.5, momentum=0.8, dampening=0.1, weight_decay=0.01)
    for size, outer in ((None, None), (3, None), (5, sgd)):
        want_rows, got_rows = [], []
        ref = DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), outer_optim_spec=outer, H=2,
                             placement=False)
        _, _, ref_runner = _replica_run(K, steps, strategy=ref,
                                        hook=lambda t, r: want_rows.append(r.ra.flat_set.numpy().copy()))
        del fake.CALLS[:]
        state = random.Random(SEED).getstate()
        _, s, runner = _replica_run(K, steps, island_size=size, outer_optim_spec=outer,
                                    hook=lambda t, r: got_rows.append(r.ra.flat_set.numpy().copy()))
        assert random.getstate() == state  # no draw
        ld = runner.ra.ld
        assert fake.CALLS == [("islands", K, ld, [[0, 1, 2]], [[0, 1, 2]], K, True)] * 3
        for t in range(steps):
            assert _same(got_rows[t], want_rows[t]), (size, t)
        for k in range(K):
            assert _same(got_rows[6][k], got_rows[6][0])  # step 6 was a round: every row the master
            assert _same(runner.outer.master[k].numpy(), ref_runner.outer.master[:ld].numpy())
            assert _same(runner.outer.mom[k].numpy(), ref_runner.outer.mom[:ld].numpy())


def test_three_nodes_the_pair_and_the_loner(fake):
    """3 nodes, islands of 2: after the first round the pair is bit-equal and the loner,
    which stepped against its own row, is not the pair."""
    rows = []
    _, s, runner = _replica_run(3, 3, island_size=2, hook=lambda t, r: rows.append(r.ra.flat_set.numpy().copy()))
    (pair, loner), = _expected_draws(3, 2, 1)
    assert len(pair) == 2 and len(loner) == 1
    assert fake.CALLS == [("islands", 3, runner.ra.ld, [pair, loner], [pair, loner], 3, True)]
    after = rows[2]
    assert _same(after[pair[0]], after[pair[1]]) and not _same(after[loner[0]], after[pair[0]])
    assert not _same(after[loner[0]], rows[1][loner[0]]) and np.isfinite(after).all()


# ------------------------------------------------------ the default paths --
def test_diloco_and_fedavg_make_the_launches_they_always_made(fake, monkeypatch):
    from gym_amd.engine import DiLoCoOuter
    from gym_amd.strategy import DiLoCoStrategy, FedAvgStrategy, OptimSpec
    ref = DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), H=2)
    _, _, runner = _replica_run(3, 5, strategy=ref)
    assert type(runner.outer) is DiLoCoOuter and fake.CALLS == [("outer", 3, runner.ra.ld)] * 2
    del fake.CALLS[:]
    torch.manual_seed(42)
    model = R._model("x", torch.device("cpu"))
    ref = DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), H=2)
    ref._init_node(model, 0, 1)
    for t in range(5):
        ref.zero_grad()
        R._set_grads(model, 0, t, torch.device("cpu"))
        ref.step()
    assert type(ref.engine) is DiLoCoOuter and fake.CALLS == [("outer", 1, ref.arena.n)] * 2
    # FedAvg's islands in replica mode: per island one table mean into the staging row, then the write-back runs
    del fake.CALLS[:]
    means = []
    orig = fake.replica_mean

    def rec(src, dst, n=None, divisor=None, rows=None):
        means.append((src.shape[0], dst.shape[0] if dst.dim() == 2 else 1, None if rows is None else rows.tolist(),
                      divisor))
        return orig(src, dst, n=n, divisor=divisor, rows=rows)

    monkeypatch.setattr(fake, "replica_mean", rec)
    fed = FedAvgStrategy(inner_optim=OptimSpec(torch.optim.SGD, lr=0.05), island_size=2, H=2)
    _replica_run(3, 3, strategy=fed)
    (pair, loner), = _expected_draws(3, 2, 1)
    want = [(1, 2, None, 1.0)]  # the runner's start: node 0's row copied to the others
    want += [(3, 1, pair, 2.0)] + [(1, 2 if pair[1] == pair[0] + 1 else 1, None, 1.0)] * (1 if pair[1] == pair[0] + 1
                                                                                       else 2)
    want += [(3, 1, loner, 1.0), (1, 1, None, 1.0)]
    assert means == want and fake.CALLS == []
    # full averaging keeps its MeanReduce
    means.clear()
    _, _, runner = _replica_run(3, 3, strategy=FedAvgStrategy(inner_optim=OptimSpec(torch.optim.SGD, lr=0.05), H=2))
    assert hasattr(runner, "mean") and not runner.islands and fake.CALLS == []
