"""The quantised DiLoCo outer step without a GPU: which options take which engine,
DiLoCoOuterQuant's plumbing against the numpy oracle (tests/quant_checks.py), two
nodes in one process against two gloo processes, SPARTA+DiLoCo with compression,
and the untouched default path -- over the stand-ins of tests/fake_quant_ops.py.
The kernels' arithmetic: test_gpu_quant_kernels.py."""
import os

import numpy as np
import pytest
import torch

import quant_checks as Q
import replica_scenarios as R

N, STEPS, H = 700, 5, 2  # three blocks, the last one short; outer steps at local_step 2 and 4
HP = dict(lr=0.7, momentum=0.9, nesterov=True, dampening=0.0, weight_decay=1e-3)
CONFIGS = [("int8", False), ("int8", True), ("int4", False), ("int4", True)]


@pytest.fixture
def fake(monkeypatch):
    """The gym_amd modules pointed at fake_quant_ops for one test (nothing set on fake_ops)."""
    import fake_quant_ops as fq
    import gym_amd.engine as engine
    import gym_amd.fused_optim as fused_optim
    import gym_amd.replica as replica
    import gym_amd.strategy.diloco as diloco
    import gym_amd.strategy.strategy as strategy
    for mod in (engine, diloco, fused_optim, replica):
        monkeypatch.setattr(mod, "ops", fq)
    monkeypatch.setattr(strategy, "require_gpu", lambda device: None)
    monkeypatch.setattr(fq, "CALLS", [])
    return fq


class Local:
    world, rank, exchange, rccl, backend = 1, 0, False, False, "none"


# ------------------------------------------------------------------ options --
def _build(strategy, K=1):
    from gym_amd.strategy import diloco
    return diloco.build_outer_engine(strategy, strategy.outer_optim_spec, Local(), K, N, "cpu", torch.float32)


def test_build_outer_engine_follows_the_options(fake):
    from gym_amd.engine import DiLoCoOuter, DiLoCoOuterAdam, DiLoCoOuterQuant, TorchOuter
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec, SPARTADiLoCoStrategy
    sgd = OptimSpec(torch.optim.SGD, lr=0.5, momentum=0.8, dampening=0.1, weight_decay=0.01)
    adam = OptimSpec(torch.optim.Adam, lr=0.05)
    assert type(_build(DiLoCoStrategy())) is DiLoCoOuter
    assert type(_build(DiLoCoStrategy(outer_error_feedback=True))) is DiLoCoOuter  # nothing to feed back
    assert type(_build(DiLoCoStrategy(outer_optim_spec=adam))) is DiLoCoOuterAdam
    assert type(_build(DiLoCoStrategy(outer_optim_spec=OptimSpec(torch.optim.RMSprop, lr=0.1)))) is TorchOuter
    e = _build(DiLoCoStrategy(outer_compression="int8"), K=3)
    assert type(e) is DiLoCoOuterQuant and not isinstance(e, DiLoCoOuter)
    assert e.bits == 8 and e.residual is None and e.hp == dict(lr=0.7, momentum=0.9, nesterov=True, dampening=0.0,
                                                               weight_decay=0.0)
    assert e.payload.shape == (3, Q.row_bytes(N, 8)) and e.payload.dtype == torch.uint8
    assert e.payload_bytes_per_node == Q.row_bytes(N, 8)
    e = _build(DiLoCoStrategy(outer_optim_spec=sgd, outer_compression="int4", outer_error_feedback=True), K=2)
    assert type(e) is DiLoCoOuterQuant and e.bits == 4 and e.residual.shape == (2, N)
    assert e.residual.dtype == torch.float32 and e.payload_bytes_per_node == Q.row_bytes(N, 4)
    assert e.hp == dict(lr=0.5, momentum=0.8, nesterov=False, dampening=0.1, weight_decay=0.01)
    assert e.master.dtype == e.mom.dtype == torch.float32 and e.master.numel() == e.mom.numel() == N  # replicated
    assert e.placement["placed"] is False and "why" in e.placement
    s = SPARTADiLoCoStrategy(outer_compression="int8", outer_error_feedback=True)
    assert s.kwargs["outer_compression"] == "int8" and s.kwargs["outer_error_feedback"] is True
    assert type(_build(s)) is DiLoCoOuterQuant and _build(s).residual is not None


@pytest.mark.parametrize("cls", ["diloco", "sparta_diloco"])
def test_compression_refuses_what_it_cannot_do(fake, cls):
    """An unknown string, or an outer optimizer without a quantised step, raises at
    construction -- and at node init when the option arrives another way; never a
    silent fallback."""
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec, SPARTADiLoCoStrategy

    def make(spec, **kw):
        if cls == "diloco":
            return DiLoCoStrategy(outer_optim_spec=spec, **kw)
        return SPARTADiLoCoStrategy(outer_optim=spec, **kw)

    for bad in ("int2", "fp8", "INT8", 8, True):
        with pytest.raises(ValueError, match="outer_compression"):
            make(None, outer_compression=bad)
    for spec in (OptimSpec(torch.optim.Adam, lr=0.05), OptimSpec(torch.optim.AdamW), "adam",
                 OptimSpec(torch.optim.RMSprop, lr=0.1), OptimSpec(torch.optim.SGD, lr=0.1, maximize=True)):
        with pytest.raises(ValueError, match="outer_compression"):
            make(spec, outer_compression="int8")
        s = make(spec)
        s.kwargs["outer_compression"] = "int4"  # set after construction: node init still refuses
        with pytest.raises(ValueError, match="outer_compression"):
            _build(s)
    s = make(None)
    s.kwargs["outer_compression"] = "int3"
    with pytest.raises(ValueError, match="outer_compression"):
        _build(s)
    assert fake.CALLS == []


def test_config_reports_both_options(fake):
    from gym_amd.strategy import DiLoCoStrategy, SPARTADiLoCoStrategy
    for make in (DiLoCoStrategy, SPARTADiLoCoStrategy):
        cfg = make().__config__()
        assert cfg["outer_compression"] is None and cfg["outer_error_feedback"] is False
        cfg = make(outer_compression="int4", outer_error_feedback=True).__config__()
        assert cfg["outer_compression"] == "int4" and cfg["outer_error_feedback"] is True


# ------------------------------------------------------------------- engine --
def _start():
    return torch.randn(N, generator=torch.Generator().manual_seed(3)) * 0.02


def _node_rows(node, step, base):
    g = torch.Generator().manual_seed(700 + 31 * node + step)
    return base + torch.randn(base.numel(), generator=g) * 1e-3


@pytest.mark.parametrize("comp,feedback", CONFIGS)
def test_engine_follows_the_oracle(fake, comp, feedback):
    """Three outer steps of three nodes in one process: payload rows in node order,
    the residual carried from step to step, master / momentum replicated, every row
    the new master, one encode and one decode launch per step."""
    from gym_amd.engine import QUANT_BITS, DiLoCoOuterQuant
    assert "REPLICATED" in DiLoCoOuterQuant.__doc__ and "not sharded" in DiLoCoOuterQuant.__doc__
    K, bits = 3, QUANT_BITS[comp]
    eng = DiLoCoOuterQuant(Local(), K, N, "cpu", torch.float32, bits=bits, error_feedback=feedback, **HP)
    eng.init_master(_start())
    assert eng.first and torch.equal(eng.master, _start()) and not eng.mom.any()
    master, mom = _start().numpy(), None
    resid = np.zeros((K, N), np.float32) if feedback else None
    x = _start().repeat(K, 1)
    for step in range(3):
        x = torch.stack([_node_rows(k, step, x[k]) for k in range(K)])
        ld = torch.full((K, N + 12), -7.25)
        ld[:, :N] = x
        pay, resid, _ = Q.encode(master, x.numpy(), resid, bits)
        master, mom, _ = Q.decode_outer(pay, N, bits, K, master, mom, HP, step == 0)
        eng(ld)
        assert np.array_equal(eng.payload.numpy(), pay)
        assert np.array_equal(eng.master.numpy().view(np.int32), master.view(np.int32))
        assert np.array_equal(eng.mom.numpy().view(np.int32), mom.view(np.int32))
        if feedback:
            assert np.array_equal(eng.residual.numpy().view(np.int32), resid.view(np.int32)) and resid.any()
        assert all(torch.equal(ld[k, :N], eng.master) for k in range(K)) and (ld[:, N:] == -7.25).all()
        assert eng.first is False and eng.launch_elems == [N]
        x = ld[:, :N].clone()
    assert fake.CALLS == [("encode", K, N, bits, feedback), ("dequant", K, N, bits, K)] * 3
    with pytest.raises(ValueError, match="no one-pass masked outer step; run Sparta and the outer step one after"):
        eng(ld, sparse_mask=torch.zeros(11, dtype=torch.int64))
    assert len(fake.CALLS) == 6
    eng.init_master(_start())
    assert eng.first and torch.equal(eng.master, _start()) and (not feedback or not eng.residual.any())
    with pytest.raises(ValueError, match="bits"):
        DiLoCoOuterQuant(Local(), 1, N, "cpu", torch.float32, bits=2)


# --------------------------------------- 2 gloo processes vs 2 nodes in one --
def _strategy(comp, feedback, kind="diloco"):
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec, SPARTADiLoCoStrategy
    inner = OptimSpec(torch.optim.AdamW, lr=1e-2)
    kw = dict(H=H, outer_compression=comp, outer_error_feedback=feedback)
    if kind == "diloco":
        return DiLoCoStrategy(optim_spec=inner, **kw)
    return SPARTADiLoCoStrategy(inner_optim=inner, p_sparta=0.1, **kw)


def _params(model):
    return [p.detach().float().numpy().copy() for p in model.parameters()]


def _gloo_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    import fake_quant_ops
    fake_quant_ops.install()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gym_amd.engine import DiLoCoOuterQuant
        out = {}
        for comp, feedback in CONFIGS:
            tag = f"{comp}_{int(feedback)}"
            torch.manual_seed(42)
            model = R._model("x", torch.device("cpu"))
            s = _strategy(comp, feedback)
            s._init_node(model, rank, world)
            assert type(s.engine) is DiLoCoOuterQuant and s.outer_optimizer is None and s.engine.K_total == world
            assert s.engine.payload.shape[0] == world and s.placement_records()["engine"]["placed"] is False
            after_outer = []
            for t in range(STEPS):
                s.zero_grad()
                R._set_grads(model, rank, t, torch.device("cpu"))
                s.step()
                if t % H == 0 and t > 0:
                    after_outer.append(s.arena.flat[:s.arena.n].numpy().copy())
            out.update({f"{tag}_{i}": p for i, p in enumerate(_params(model))})
            out[f"{tag}_outer"] = np.stack(after_outer)
            out[f"{tag}_payload"] = s.engine.payload.numpy().copy()
        np.savez(os.path.join(out_dir, f"q{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def _replica_run(comp, feedback, K=2, kind="diloco"):
    from gym_amd.replica import ReplicaRunner
    torch.manual_seed(42)
    dev = torch.device("cpu")
    models = [R._model("x", dev) for _ in range(K)]
    s = _strategy(comp, feedback, kind)
    runner = ReplicaRunner(s, models, rank=0, num_nodes=K)
    after_outer = []
    for t in range(STEPS):
        runner.zero_grad()
        for k, m in enumerate(models):
            R._set_grads(m, k, t, dev)
        runner.step()
        if t % H == 0 and t > 0:
            after_outer.append(runner.ra.flat_set[:, :runner.ra.arenas[0].n].numpy().copy())
    return [_params(m) for m in models], s, runner, after_outer


def test_two_nodes_in_one_process_equal_two_gloo_processes(tmp_path, fake):
    """DiLoCoStrategy over 2 gloo processes against ReplicaRunner with both nodes in
    one process, int8 and int4, with and without error feedback, two outer steps:
    the same payload bytes decoded in the same order, so every node's parameters
    are bit-identical between the modes, and equal across the nodes after each
    outer step."""
    import torch.multiprocessing as mp
    from strategy_scenarios import free_port
    from gym_amd.engine import DiLoCoOuterQuant
    mp.spawn(_gloo_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    res = [dict(np.load(tmp_path / f"q{r}.npz")) for r in range(2)]
    seen = []
    for comp, feedback in CONFIGS:
        tag = f"{comp}_{int(feedback)}"
        del fake.CALLS[:]
        nodes, s, runner, after_outer = _replica_run(comp, feedback)
        eng = runner.outer
        assert type(eng) is DiLoCoOuterQuant and (eng.residual is not None) is feedback
        n, bits = eng.n, eng.bits
        assert fake.CALLS == [("encode", 2, n, bits, feedback), ("dequant", 2, n, bits, 2)] * 2
        assert len(after_outer) == 2
        for r in range(2):
            for i, p in enumerate(nodes[r]):
                assert np.array_equal(res[r][f"{tag}_{i}"].view(np.int32), p.view(np.int32)), (tag, r, i)
            assert np.array_equal(res[r][f"{tag}_payload"], eng.payload.numpy()), (tag, r)
            for j, rows in enumerate(after_outer):  # every node equal after each outer step, in both modes
                assert np.array_equal(rows[0], rows[1]) and np.array_equal(res[r][f"{tag}_outer"][j], rows[0])
        assert not np.array_equal(nodes[0][0], R._model("x", torch.device("cpu")).ps[0].detach().numpy())
        seen.append(np.concatenate([p.reshape(-1) for p in nodes[0]]))
    for a in range(len(seen)):  # the four configurations are four different runs
        for b in range(a):
            assert not np.array_equal(seen[a], seen[b])


# ------------------------------------------------------------ SPARTA+DiLoCo --
def test_sparta_diloco_with_compression_runs_the_modules_in_sequence(fake):
    from gym_amd.engine import DiLoCoOuterQuant
    nodes, s, runner, _ = _replica_run("int8", True, K=3, kind="sparta")
    assert s.fuse_boundary is False and runner.fuse is False and s.__config__()["fuse_boundary"] is False
    assert type(runner.outer) is DiLoCoOuterQuant and s.engine is runner.outer
    assert s.placement_records()["engine"] == runner.outer.placement and runner.outer.placement["placed"] is False
    kinds = [c[0] for c in fake.CALLS]
    assert kinds == ["encode", "dequant"] * 2 and "masked" not in kinds and "outer" not in kinds
    for k in range(1, 3):  # the last step is an outer step: every node holds the master
        for a, b in zip(nodes[0], nodes[k]):
            assert np.array_equal(a, b)
    # without the option the boundary steps take the masked one-pass step, as before
    del fake.CALLS[:]
    _, s0, runner0, _ = _replica_run(None, False, K=3, kind="sparta")
    assert s0.fuse_boundary is True and [c[0] for c in fake.CALLS] == ["masked", "masked"]


# ------------------------------------------------------- the default path --
def test_options_unset_make_the_launches_they_always_made(fake):
    """DiLoCo with no compression: one ga_diloco_outer launch over the K rows per outer
    step and nothing else -- no encode, no decode, no payload."""
    from gym_amd.engine import DiLoCoOuter
    _, s, runner, _ = _replica_run(None, False, K=3)
    assert type(runner.outer) is DiLoCoOuter and not hasattr(runner.outer, "payload")
    assert fake.CALLS == [("outer", 3, runner.ra.ld)] * 2
    del fake.CALLS[:]
    _, s, runner, _ = _replica_run(None, True, K=2)  # feedback alone changes nothing
    assert type(runner.outer) is DiLoCoOuter and fake.CALLS == [("outer", 2, runner.ra.ld)] * 2
    # process mode, one node
    del fake.CALLS[:]
    torch.manual_seed(42)
    model = R._model("x", torch.device("cpu"))
    s = _strategy(None, False)
    s._init_node(model, 0, 1)
    for t in range(STEPS):
        s.zero_grad()
        R._set_grads(model, 0, t, torch.device("cpu"))
        s.step()
    assert type(s.engine) is DiLoCoOuter and fake.CALLS == [("outer", 1, s.arena.n)] * 2
