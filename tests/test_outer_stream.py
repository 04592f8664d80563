"""Streaming DiLoCo without a GPU: the options and what they select, where the arena
is cut, when the fragments fire, FragmentedOuter / DiLoCoOuterStream against the numpy
replay (tests/stream_checks.py), two nodes in one process against two gloo processes,
and the untouched default path -- over the stand-ins of tests/fake_stream_ops.py.
The kernel's arithmetic: test_gpu_outer_stream_kernels.py."""
import os

import numpy as np
import pytest
import torch

import replica_scenarios as R
import stream_checks as S

f32 = np.float32
HP = dict(lr=0.7, momentum=0.9, nesterov=True, dampening=0.0, weight_decay=1e-3)


@pytest.fixture
def fake(monkeypatch):
    """The gym_amd modules pointed at fake_stream_ops for one test, one fresh CALLS list."""
    import fake_quant_ops as fq
    import fake_stream_ops as fs
    import gym_amd.engine as engine
    import gym_amd.fused_optim as fused_optim
    import gym_amd.replica as replica
    import gym_amd.strategy.diloco as diloco
    import gym_amd.strategy.strategy as strategy
    for mod in (engine, diloco, fused_optim, replica):
        monkeypatch.setattr(mod, "ops", fs)
    monkeypatch.setattr(strategy, "require_gpu", lambda device: None)
    calls = []
    monkeypatch.setattr(fq, "CALLS", calls)
    monkeypatch.setattr(fs, "CALLS", calls)
    return fs


class Local:
    world, rank, exchange, rccl, backend = 1, 0, False, False, "none"


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, f32)).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ options --
def test_options_are_validated_at_construction(fake):
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    adam = OptimSpec(torch.optim.Adam, lr=0.05)
    for bad in (0, -1, 7, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="num_fragments"):
            DiLoCoStrategy(H=6, num_fragments=bad)
    for bad in (-1, 6, 9, 1.0, "1", True, None):
        with pytest.raises(ValueError, match="outer_delay"):
            DiLoCoStrategy(H=6, outer_delay=bad)
    for bad in (-0.1, 1.0, 1.5, float("nan"), "0.5", True, None):
        with pytest.raises(ValueError, match="outer_mix"):
            DiLoCoStrategy(H=6, outer_mix=bad)
    for kw in (dict(outer_delay=1), dict(outer_mix=0.5), dict(outer_delay=2, outer_mix=0.25, num_fragments=3)):
        for spec in (adam, OptimSpec(torch.optim.AdamW), OptimSpec(torch.optim.RMSprop, lr=0.1),
                     OptimSpec(torch.optim.SGD, lr=0.1, maximize=True)):
            with pytest.raises(ValueError, match="plain torch.optim.SGD"):
                DiLoCoStrategy(H=6, outer_optim_spec=spec, **kw)
        with pytest.raises(ValueError, match="outer_compression"):
            DiLoCoStrategy(H=6, outer_compression="int8", **kw)
    s = DiLoCoStrategy(H=6, num_fragments=6, outer_delay=5, outer_mix=0.999)  # the ends of the ranges
    assert s.kwargs["num_fragments"] == 6 and s.kwargs["outer_delay"] == 5 and s.kwargs["outer_mix"] == 0.999
    assert s.num_fragments == 6 and s.outer_delay == 5
    cfg = s.__config__()
    assert cfg["num_fragments"] == 6 and cfg["outer_delay"] == 5 and cfg["outer_mix"] == 0.999
    cfg = DiLoCoStrategy().__config__()
    assert cfg["num_fragments"] == 1 and cfg["outer_delay"] == 0 and cfg["outer_mix"] == 0.0
    # fragments alone compose with Adam and with compression
    DiLoCoStrategy(H=6, num_fragments=3, outer_optim_spec=adam)
    DiLoCoStrategy(H=6, num_fragments=3, outer_compression="int4")
    s = DiLoCoStrategy(H=6)
    s.kwargs["outer_delay"] = 6  # set after construction: node init still refuses
    with pytest.raises(ValueError, match="outer_delay"):
        s._init_node(R._model("x", torch.device("cpu")), 0, 1)
    assert fake.CALLS == []


def test_sparta_diloco_does_not_take_the_options(fake):
    """SPARTADiLoCoStrategy is unchanged: the names are unknown kwargs there, kept as
    attributes as every unknown kwarg is, and its outer step stays DiLoCoOuter's."""
    from gym_amd.engine import DiLoCoOuter
    from gym_amd.strategy import diloco, SPARTADiLoCoStrategy
    s = SPARTADiLoCoStrategy(H=4, num_fragments=2, outer_delay=1, outer_mix=0.5)
    assert diloco.streaming_options(s, s.outer_optim_spec) is None
    e = diloco.build_outer_engine(s, s.outer_optim_spec, Local(), 2, 1024, "cpu", torch.float32)
    assert type(e) is DiLoCoOuter


# ------------------------------------------------------- the default path --
STEPS, H = 5, 2


def _strategy(**kw):
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    kw.setdefault("H", H)
    return DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), **kw)


def _params(model):
    return [p.detach().float().numpy().copy() for p in model.parameters()]


def _replica_run(K=2, steps=STEPS, hook=None, **kw):
    from gym_amd.replica import ReplicaRunner
    torch.manual_seed(42)
    dev = torch.device("cpu")
    models = [R._model("x", dev) for _ in range(K)]
    s = _strategy(**kw)
    runner = ReplicaRunner(s, models, rank=0, num_nodes=K)
    for t in range(steps):
        runner.zero_grad()
        for k, m in enumerate(models):
            R._set_grads(m, k, t, dev)
        runner.step()
        if hook is not None:
            hook(t, runner)
    return [_params(m) for m in models], s, runner


def test_defaults_build_the_engines_and_make_the_launches_they_always_made(fake):
    from gym_amd.engine import DiLoCoOuter, FragmentedOuter
    from gym_amd.strategy import diloco
    s = _strategy()
    assert diloco.streaming_options(s, s.outer_optim_spec) is None
    _, s, runner = _replica_run(K=3)
    assert type(runner.outer) is DiLoCoOuter and not isinstance(runner.outer, FragmentedOuter)
    assert fake.CALLS == [("outer", 3, runner.ra.ld)] * 2
    runner.finish()  # nothing to finish
    del fake.CALLS[:]
    _, s, runner = _replica_run(K=2, num_fragments=1, outer_delay=0, outer_mix=0.0)  # spelled out: the same
    assert type(runner.outer) is DiLoCoOuter and fake.CALLS == [("outer", 2, runner.ra.ld)] * 2
    # process mode, one node
    del fake.CALLS[:]
    torch.manual_seed(42)
    model = R._model("x", torch.device("cpu"))
    s = _strategy()
    s._init_node(model, 0, 1)
    for t in range(STEPS):
        s.zero_grad()
        R._set_grads(model, 0, t, torch.device("cpu"))
        s.step()
    s.finish()
    assert type(s.engine) is DiLoCoOuter and fake.CALLS == [("outer", 1, s.arena.n)] * 2


# ----------------------------------------------------------- the fragments --
OFFSETS = [0, 1000, 2000, 2500, 3000, 5000]  # a hand-made layout of n = 6144 elements


def test_fragment_bounds_on_a_hand_made_layout():
    from gym_amd.engine import fragment_bounds
    n = 6144
    assert fragment_bounds(OFFSETS, n, 1, 512) == [0, n]
    # n / 2 = 3072: the tensor at 3000; rounded down to 512: 2560 (inside the tensor at 2500)
    assert fragment_bounds(OFFSETS, n, 2, 512) == [0, 2560, n]
    assert fragment_bounds(OFFSETS, n, 2, 1) == [0, 3000, n]
    # thirds 2048 and 4096: 2000 (48 away, 2500 is 452); 4096 is 1096 from 3000 and 904 from 5000
    assert fragment_bounds(OFFSETS, n, 3, 1) == [0, 2000, 5000, n]
    assert fragment_bounds(OFFSETS, n, 3, 512) == [0, 1536, 4608, n]
    # a tie goes to the lower tensor: 2250 is 250 from both 2000 and 2500
    assert fragment_bounds([0, 2000, 2500], 4500, 2, 1) == [0, 2000, 4500]
    assert fragment_bounds([0, 2000, 2500], 4500, 2, 500) == [0, 2000, 4500]
    assert fragment_bounds(reversed(OFFSETS), n, 2, 512) == [0, 2560, n]  # any order of the offsets
    for F in (1, 2, 3):
        for unit in (1, 500, 512):
            assert fragment_bounds(OFFSETS, n, F, unit) == S.bounds(OFFSETS, n, F, unit)
    # too many fragments: two cuts at one tensor, a cut rounded down to 0, a cut at n
    for offs, F, unit in ((OFFSETS, 6, 1), (OFFSETS, 4, 2048), ([0, 100], 2, 512), ([0], 2, 1), ([0, 6144], 2, 1)):
        assert S.bounds(offs, n, F, unit) is None
        with pytest.raises(ValueError, match="num_fragments too large for this model"):
            fragment_bounds(offs, n, F, unit)


@pytest.mark.parametrize("H_,F", [(6, 3), (5, 2)])
def test_schedule(H_, F):
    """Every fragment fires once per H steps, fragment 0 on DiLoCo's steps, none at step 0."""
    from gym_amd.engine import FragmentedOuter

    class Rec:
        placement = None

        def __init__(self):
            self.calls, self.launch_elems = [], [1]

        def __call__(self, reps):
            self.calls.append(self.t)

    engines = [Rec() for _ in range(F)]
    fo = FragmentedOuter(engines, list(range(0, 8 * (F + 1), 8)), H_, 0)
    reps = torch.zeros(1, 8 * F)
    for t in range(4 * H_ + 1):
        for e in engines:
            e.t = t
        fo.step(reps, t)
        assert len(fo.launch_elems) == sum(S.fires(f, t, H_, F) for f in range(F))
    for f, e in enumerate(engines):
        assert e.calls == [t for t in range(4 * H_ + 1) if S.fires(f, t, H_, F)] and 0 not in e.calls
        for p in range(1 if f == 0 else 0, 4):  # once in every window of H steps (fragment 0 skips step 0)
            assert sum(p * H_ <= t < (p + 1) * H_ for t in e.calls) == 1, (f, p, e.calls)
        assert all(b - a == H_ for a, b in zip(e.calls, e.calls[1:]))
    assert engines[0].calls == [t for t in range(1, 4 * H_ + 1) if t % H_ == 0]  # DiLoCo's steps
    firsts = sorted(e.calls[0] % H_ for e in engines)
    assert len(set(firsts)) == F  # staggered: no two fragments share a step
    if (H_, F) == (6, 3):
        assert [e.calls[:2] for e in engines] == [[6, 12], [4, 10], [2, 8]]
    else:
        assert [e.calls[:2] for e in engines] == [[5, 10], [3, 8]]


def test_engine_selection_per_option(fake):
    from gym_amd.engine import (DiLoCoOuter, DiLoCoOuterAdam, DiLoCoOuterQuant, DiLoCoOuterStream, FragmentedOuter,
                                TorchOuter)
    from gym_amd.strategy import OptimSpec, diloco
    n = 6144

    def build(K=2, **kw):
        s = _strategy(**kw)
        opts = diloco.streaming_options(s, s.outer_optim_spec)
        assert opts == (s.kwargs["num_fragments"], s.kwargs["outer_delay"], s.kwargs["outer_mix"])
        return diloco.build_streaming_outer(s, s.outer_optim_spec, Local(), K, n, "cpu", torch.float32, OFFSETS, opts)

    sgd = OptimSpec(torch.optim.SGD, lr=0.5, momentum=0.8, dampening=0.1, weight_decay=0.01)
    cases = [(dict(num_fragments=3, H=6), DiLoCoOuter),
             (dict(num_fragments=3, H=6, outer_optim_spec=OptimSpec(torch.optim.Adam, lr=0.05)), DiLoCoOuterAdam),
             (dict(num_fragments=3, H=6, outer_compression="int8", outer_error_feedback=True), DiLoCoOuterQuant),
             (dict(num_fragments=3, H=6, outer_delay=2), DiLoCoOuterStream),
             (dict(num_fragments=3, H=6, outer_mix=0.5), DiLoCoOuterStream),
             (dict(H=6, outer_delay=1, outer_mix=0.25, outer_optim_spec=sgd), DiLoCoOuterStream)]
    for kw, cls in cases:
        fo = build(**kw)
        F = kw.get("num_fragments", 1)
        assert type(fo) is FragmentedOuter and fo.H == 6 and fo.delay == kw.get("outer_delay", 0)
        assert fo.bounds == S.bounds(OFFSETS, n, F, 512) and len(fo.engines) == F
        assert fo.placement["placed"] is False and "why" in fo.placement and fo.launch_elems == []
        for f, e in enumerate(fo.engines):
            assert type(e) is cls and e.n == fo.bounds[f + 1] - fo.bounds[f] and e.K_local == 2
            assert e.master.dtype == torch.float32 and e.master.numel() == e.n
            if cls is DiLoCoOuter:
                assert e.place_opt is False
            if cls is DiLoCoOuterQuant:
                assert e.bits == 8 and e.residual.shape == (2, e.n)
            if cls is DiLoCoOuterStream:
                assert e.delay == kw.get("outer_delay", 0) and e.mix == kw.get("outer_mix", 0.0)
                assert (e.stage is not None) == (e.delay > 0) and e.placement["placed"] is False
                assert e.mom.numel() == e.n and "REPLICATED" in DiLoCoOuterStream.__doc__
    assert build(H=6, outer_delay=1, outer_mix=0.25, outer_optim_spec=sgd).engines[0].hp == dict(
        lr=0.5, momentum=0.8, nesterov=False, dampening=0.1, weight_decay=0.01)
    for spec in (OptimSpec(torch.optim.RMSprop, lr=0.1), OptimSpec(torch.optim.SGD, lr=0.1, maximize=True)):
        with pytest.raises(ValueError, match="num_fragments=2 needs a fused outer step"):
            build(num_fragments=2, H=6, outer_optim_spec=spec)
    with pytest.raises(ValueError, match="needs a fused outer step"):  # Adam kept on torch's optimizer
        build(num_fragments=2, H=6, outer_optim_spec=OptimSpec(torch.optim.Adam, lr=0.05), fused_outer=False)
    with pytest.raises(ValueError, match="num_fragments too large for this model"):
        build(num_fragments=6, H=6)
    assert type(diloco.build_outer_engine(_strategy(outer_optim_spec=OptimSpec(torch.optim.RMSprop, lr=0.1)),
                                          OptimSpec(torch.optim.RMSprop, lr=0.1), Local(), 1, n, "cpu",
                                          torch.float32)) is TorchOuter
    with pytest.raises(ValueError, match="no one-pass masked outer step"):
        build(H=6, outer_mix=0.5).engines[0](torch.zeros(2, n), sparse_mask=torch.zeros(96, dtype=torch.int64))
    assert fake.CALLS == []


# ------------------------------------------- FragmentedOuter against run() --
CUTS = [0, 1024, 1536, 2560]


def _deltas(K, n, steps, seed=5, scale=1e-3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((steps, K, n)) * scale).astype(f32)


def _stream_outer(K, cuts, H_, delay, mix, coll=None, dtype=torch.float32, hp=HP):
    from gym_amd.comm import Collective
    from gym_amd.engine import DiLoCoOuterStream, FragmentedOuter
    engines = [DiLoCoOuterStream(coll or Collective(), K, b - a, "cpu", dtype, delay=delay, mix=mix, **hp)
               for a, b in zip(cuts, cuts[1:])]
    return FragmentedOuter(engines, cuts, H_, delay)


def test_fragmented_outer_follows_the_replay(fake):
    """K = 3, three fragments, H = 6, tau = 2, alpha = 0.5, 14 steps with the rows
    perturbed on every step: rows, master and momentum bit for bit after every step,
    every merge exactly tau steps after its send."""
    K, n, H_, tau, alpha, steps = 3, CUTS[-1], 6, 2, 0.5, 14
    rng = np.random.default_rng(2)
    x0 = np.tile((rng.standard_normal(n) * 0.02).astype(f32), (K, 1))
    deltas = _deltas(K, n, steps)
    want = S.run(x0, deltas, CUTS, H_, tau, alpha, HP)
    fo = _stream_outer(K, CUTS, H_, tau, alpha)
    reps = torch.full((K, n + 12), -7.25)
    reps[:, :n] = torch.from_numpy(x0)
    fo.init_master(reps[0])
    sends, merges = {}, {}
    for t in range(steps):
        reps[:, :n] += torch.from_numpy(deltas[t])
        before = len(fake.CALLS)
        fo.step(reps, t)
        w = want[t]
        assert _same(reps[:, :n].numpy(), w["rows"]), t
        master = np.concatenate([e.master.numpy() for e in fo.engines])
        mom = np.concatenate([e.mom.numpy() for e in fo.engines])
        assert _same(master, w["master"]) and _same(mom, w["mom"]), t
        assert (reps[:, n:] == -7.25).all()
        new = fake.CALLS[before:]
        for kind, f in w["events"]:
            (sends if kind == "send" else merges).setdefault(f, []).append(t)
        lens = [CUTS[f + 1] - CUTS[f] for kind, f in w["events"] if kind == "merge"]
        assert new == [("merge", 1, ln, K, alpha, False) for ln in lens]  # one launch per merge, off the staged sum
        assert fo.launch_elems == lens
    assert sends == {0: [6, 12], 1: [4, 10], 2: [2, 8]}
    assert merges == {0: [8], 1: [6, 12], 2: [4, 10]}  # fragment 0's second merge is still pending at the end
    assert fo.due == [14, None, None]
    rows = w["rows"]
    assert not _same(rows[0], rows[1])  # mixed, not overwritten: the nodes keep their own progress
    # finish(): the pending merge is dropped, the rows stay as they are
    kept, state = reps.clone(), [e.master.clone() for e in fo.engines]
    before = len(fake.CALLS)
    fo.finish()
    assert fo.due == [None] * 3 and len(fake.CALLS) == before and torch.equal(reps, kept)
    assert all(torch.equal(a, e.master) for a, e in zip(state, fo.engines))
    fo.step(reps, 14)  # nothing lands after finish()
    assert len(fake.CALLS) == before and torch.equal(reps, kept)


def test_one_fragment_no_delay_no_mix_is_diloco_outer(fake):
    """F = 1, tau = 0, alpha = 0 through FragmentedOuter and DiLoCoOuterStream: one in-place
    merge launch per outer step and no staging row, bit-identical to DiLoCoOuter over a
    whole run, in fp32 and on a bf16 set."""
    from gym_amd.engine import DiLoCoOuter
    K, n, H_, steps = 3, 2560, 4, 13
    for dtype in (torch.float32, torch.bfloat16):
        x0 = torch.from_numpy(np.tile((np.random.default_rng(3).standard_normal(n) * 0.02).astype(f32), (K, 1)))
        deltas = torch.from_numpy(_deltas(K, n, steps, scale=1e-2))
        a = x0.to(dtype).clone()
        b = a.clone()
        fo = _stream_outer(K, [0, n], H_, 0, 0.0, dtype=dtype)
        assert fo.engines[0].stage is None
        ref = DiLoCoOuter(Local(), K, n, "cpu", dtype, placement=False, **HP)
        fo.init_master(a[0].float())
        ref.init_master(b[0].float())
        del fake.CALLS[:]
        for t in range(steps):
            a += deltas[t].to(dtype)
            b += deltas[t].to(dtype)
            fo.step(a, t)
            if t % H_ == 0 and t > 0:
                ref(b)
            assert torch.equal(a, b), (dtype, t)
            assert torch.equal(fo.engines[0].master, ref.master) and torch.equal(fo.engines[0].mom, ref.mom)
        assert fake.CALLS == [("merge", K, n, K, 0.0, True), ("outer", K, n)] * 3
        assert torch.equal(a[0], a[1]) and torch.equal(a[0], a[2])  # step 12 was an outer step: every row the master


# --------------------------------------- 2 gloo processes vs 2 nodes in one --
STREAM_KW = dict(H=4, num_fragments=2, outer_delay=1, outer_mix=0.5)
GLOO_STEPS = 10


def _gloo_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    import fake_stream_ops
    fake_stream_ops.install()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gym_amd.engine import DiLoCoOuterStream, FragmentedOuter
        torch.manual_seed(42)
        model = R._model("x", torch.device("cpu"))
        s = _strategy(**STREAM_KW)
        s._init_node(model, rank, world)
        assert type(s.engine) is FragmentedOuter and s.outer_optimizer is None
        assert all(type(e) is DiLoCoOuterStream and e.K_total == world for e in s.engine.engines)
        assert s.placement_records()["engine"]["placed"] is False
        rows = []
        for t in range(GLOO_STEPS):
            s.zero_grad()
            R._set_grads(model, rank, t, torch.device("cpu"))
            s.step()
            rows.append(s.arena.flat[:s.arena.n].numpy().copy())
        s.finish()
        out = {f"p{i}": p for i, p in enumerate(_params(model))}
        np.savez(os.path.join(out_dir, f"s{rank}.npz"), rows=np.stack(rows), bounds=np.array(s.engine.bounds), **out)
    finally:
        dist.destroy_process_group()


def test_two_nodes_in_one_process_equal_two_gloo_processes(tmp_path, fake):
    """DiLoCoStrategy(H=4, F=2, tau=1, alpha=0.5) over 2 gloo processes against
    ReplicaRunner with both nodes in one process, 10 steps: the staged sum of two rows
    has one order, so every node's parameters are bit-identical between the modes on
    every step."""
    import torch.multiprocessing as mp
    from strategy_scenarios import free_port
    from gym_amd.engine import DiLoCoOuterStream, FragmentedOuter
    mp.spawn(_gloo_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    res = [dict(np.load(tmp_path / f"s{r}.npz")) for r in range(2)]
    rows = []
    nodes, s, runner = _replica_run(K=2, steps=GLOO_STEPS,
                                    hook=lambda t, r: rows.append(r.ra.flat_set[:, :r.ra.ld].numpy().copy()),
                                    **STREAM_KW)
    fo = runner.outer
    assert type(fo) is FragmentedOuter and all(type(e) is DiLoCoOuterStream for e in fo.engines)
    assert fo.bounds == [0, 2048, runner.ra.ld] == list(res[0]["bounds"]) == list(res[1]["bounds"])
    for r in range(2):
        for t in range(GLOO_STEPS):
            assert _same(res[r]["rows"][t], rows[t][r]), (r, t)
        for i, p in enumerate(nodes[r]):
            assert _same(res[r][f"p{i}"], p), (r, i)
    # fragment 0 sends at 4, 8 and merges at 5, 9; fragment 1 sends at 2, 6 and merges at 3, 7
    lens = {0: 2048, 1: runner.ra.ld - 2048}
    merges = [c for c in fake.CALLS if c[0] == "merge"]
    assert merges == [("merge", 1, lens[f], 2, 0.5, False) for f in (1, 0, 1, 0)]
    assert not any(c[0] == "outer" for c in fake.CALLS)
    a, b = rows[9][0], rows[9][1]
    assert not np.array_equal(a[:2048], b[:2048])  # mixed at step 9, not overwritten
    runner.finish()
    assert fo.due == [None, None]


def test_finish_with_a_merge_pending_leaves_the_rows_unchanged(fake):
    """Process mode: fragment 1 sends at step 2 of H = 4 and training ends there."""
    torch.manual_seed(42)
    model = R._model("x", torch.device("cpu"))
    s = _strategy(**STREAM_KW)
    s._init_node(model, 0, 1)
    for t in range(3):
        s.zero_grad()
        R._set_grads(model, 0, t, torch.device("cpu"))
        s.step()
    fo = s.engine
    assert fo.due == [None, 3] and not any(c[0] == "merge" for c in fake.CALLS)
    kept = s.arena.flat.clone()
    n_calls = len(fake.CALLS)
    s.finish()
    assert fo.due == [None, None] and torch.equal(s.arena.flat, kept) and len(fake.CALLS) == n_calls
    assert all(e._work is None for e in fo.engines)
