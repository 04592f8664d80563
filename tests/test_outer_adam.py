"""The fused Adam / AdamW outer step without a GPU: which specs take it
(fused_adam_hparams), the engine's step count and bias corrections, the gloo and
sharded branches against replicas in one process, the strategies' wiring and
the C ABI's argument checks -- over the oracle-backed stand-ins of
tests/fake_outer_adam_ops.py.  The kernel's arithmetic: test_gpu_outer_adam.py."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import outer_adam_checks as C
import replica_scenarios as R
import sparta_diloco_scenarios as SD
from oracle.reduce import mean_reduce

N, STEPS = 512, 3
HP = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, decoupled=True)


@pytest.fixture
def fake(monkeypatch):
    """The gym_amd modules pointed at fake_outer_adam_ops for one test (nothing set on fake_ops)."""
    import fake_outer_adam_ops as foa
    import gym_amd.engine as engine
    import gym_amd.fused_optim as fused_optim
    import gym_amd.replica as replica
    import gym_amd.strategy.diloco as diloco
    import gym_amd.strategy.strategy as strategy
    for mod in (engine, diloco, fused_optim, replica):
        monkeypatch.setattr(mod, "ops", foa)
    monkeypatch.setattr(strategy, "require_gpu", lambda device: None)
    monkeypatch.setattr(foa, "CALLS", [])
    return foa


class Local:
    world, rank, exchange, rccl, backend = 1, 0, False, False, "none"


# ------------------------------------------------------------------- specs --
def test_fused_adam_hparams_table(monkeypatch):
    import gym_amd.ops
    import gym_amd.strategy.diloco as diloco
    from gym_amd.strategy import OptimSpec
    from gym_amd.strategy.diloco import fused_adam_hparams, fused_sgd_hparams
    monkeypatch.setattr(diloco, "ops", gym_amd.ops)  # the product's kernel layer, whatever a stand-in left installed
    A, W = torch.optim.Adam, torch.optim.AdamW
    assert fused_adam_hparams(OptimSpec(A)) == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                                                    decoupled=False)
    assert fused_adam_hparams(OptimSpec(W)) == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                                                    decoupled=True)
    assert fused_adam_hparams(OptimSpec.from_string("adam", lr=0.05))["lr"] == 0.05
    assert fused_adam_hparams(OptimSpec.from_string("adamw"))["decoupled"] is True
    got = fused_adam_hparams(OptimSpec(A, lr=0.1, betas=(0.3, 0.9), eps=1e-6, weight_decay=0.2, foreach=True,
                                       fused=None))
    assert got == dict(lr=0.1, betas=(0.3, 0.9), eps=1e-6, weight_decay=0.2, decoupled=False)
    for bad in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True),
                dict(lr=torch.tensor(0.1)), dict(decoupled_weight_decay=True), dict(spam=1),
                dict(amsgrad=False)):  # any kwarg outside the accepted six keeps torch's optimizer
        assert fused_adam_hparams(OptimSpec(A, **bad)) is None, bad
        assert fused_adam_hparams(OptimSpec(W, **bad)) is None, bad
    for cls in (torch.optim.SGD, torch.optim.RMSprop, torch.optim.Adagrad, torch.optim.Adamax):
        assert fused_adam_hparams(OptimSpec(cls, lr=0.1)) is None
    assert fused_sgd_hparams(OptimSpec(A)) is None and fused_sgd_hparams(OptimSpec(W)) is None


def test_a_kernel_layer_without_the_op_keeps_torch(monkeypatch):
    """The hasattr rule: tests/fake_ops.py was written before ga_diloco_outer_adam."""
    import fake_ops
    import gym_amd.strategy.diloco as diloco
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    import gym_amd.ops
    spec = OptimSpec(torch.optim.Adam, lr=0.05)
    monkeypatch.setattr(diloco, "ops", gym_amd.ops)
    assert diloco.fused_adam_hparams(spec) is not None  # gym_amd.ops has the op
    assert not hasattr(fake_ops, "diloco_outer_adam")
    monkeypatch.setattr(diloco, "ops", fake_ops)
    assert diloco.fused_adam_hparams(spec) is None
    from gym_amd.engine import TorchOuter
    assert type(diloco.build_outer_engine(DiLoCoStrategy(outer_optim_spec=spec), spec, Local(), 1, N, "cpu",
                                          torch.float32)) is TorchOuter


def test_ops_and_abi_symbols():
    from gym_amd import _lib, ops
    assert callable(ops.diloco_outer_adam) and callable(ops.diloco_outer_adam_masked)
    syms = _lib.header_symbols()
    for name in ("ga_diloco_outer_adam", "ga_diloco_outer_adam_masked"):
        assert name in syms and name in _lib.SIGNATURES
    assert _lib.lib().ga_abi_version() == 103


# ------------------------------------------------------------------ engine --
def _rows(K, n, seed, master):
    g = torch.Generator().manual_seed(seed)
    return master + torch.randn(K, n, generator=g) * 1e-3


def test_engine_counts_steps_and_follows_the_bias_corrections(fake):
    from gym_amd.engine import DiLoCoOuter, DiLoCoOuterAdam
    K = 3
    eng = DiLoCoOuterAdam(Local(), K, N, "cpu", torch.float32, **HP)
    assert isinstance(eng, DiLoCoOuter) and eng.mom is None and eng.first is True and eng.per == N
    assert eng._state.numel() == 3 * N and eng._state.dtype == torch.float32
    for i, part in enumerate((eng.master, eng.exp_avg, eng.exp_avg_sq)):
        assert part.data_ptr() == eng._state.data_ptr() + 4 * i * N
    start = torch.randn(N, generator=torch.Generator().manual_seed(1)) * 0.02
    eng.init_master(start)
    for step in range(1, STEPS + 1):
        reps = _rows(K, N, 10 + step, eng.master)
        reps[:, :8] = eng.master[:8]  # g == 0 there
        pre = [x.clone() for x in (eng.master, eng.exp_avg, eng.exp_avg_sq)]
        rows0 = reps.clone()
        sc = eng.scalars(step)
        assert sc["step_size"] == -(HP["lr"] / (1 - 0.9 ** step)) and sc["bc2_sqrt"] == math.sqrt(1 - 0.999 ** step)
        assert (sc["lerp_w"], sc["beta2"], sc["one_m_beta2"]) == (1 - 0.9, 0.999, 1 - 0.999)
        assert sc["wd_factor"] == 1 - 0.05 * 0.01 and sc["l2_wd"] == 0.0
        eng(reps)
        assert eng.t == step and eng.first is False and eng.launch_elems == [N]
        assert eng.placement == {"placed": False, "why": "no search for the Adam outer step (three state streams)"}
        got = [x.numpy() for x in (eng.master, eng.exp_avg, eng.exp_avg_sq)]
        want = C.oracle_step(rows0.numpy(), K, *[x.numpy() for x in pre], step, HP)
        C.assert_step(got, want, f"step {step} vs oracle")
        avg = torch.from_numpy(mean_reduce(list(rows0.numpy()), divisor=K))
        C.assert_step(got, C.torch_step(torch.optim.AdamW, dict(lr=0.05, weight_decay=0.01), *pre, step - 1, avg),
                      f"step {step} vs torch.optim.AdamW")
        for k in range(K):
            assert torch.equal(reps[k], eng.master)
        if step == 1:
            assert np.array_equal(got[0][:8], (pre[0].numpy()[:8] * np.float32(1 - 0.05 * 0.01)))
    eng.init_master(start)
    assert eng.t == 0 and eng.first is True and torch.equal(eng.master, start)
    assert not eng.exp_avg.any() and not eng.exp_avg_sq.any()


def test_adam_l2_scalars():
    from gym_amd.engine import DiLoCoOuterAdam
    eng = DiLoCoOuterAdam(Local(), 1, 64, "cpu", torch.float32, lr=0.1, weight_decay=0.2, decoupled=False)
    sc = eng.scalars(4)
    assert sc["wd_factor"] == 1.0 and sc["l2_wd"] == 0.2
    assert DiLoCoOuterAdam(Local(), 1, 64, "cpu", torch.float32).scalars(1)["l2_wd"] == 0.0


def test_masked_step_needs_a_local_step_and_leaves_the_count(fake):
    from gym_amd.engine import DiLoCoOuterAdam

    class Exchanging:
        world, rank, exchange, rccl, backend = 2, 0, True, False, "gloo"

    eng = DiLoCoOuterAdam(Exchanging(), 1, 128, "cpu", torch.float32)
    with pytest.raises(ValueError, match="no-exchange"):
        eng(torch.zeros(1, 128), sparse_mask=torch.zeros(2, dtype=torch.int64))
    assert eng.t == 0 and fake.CALLS == []


# ------------------------------------------------- 2 gloo processes, shards --
def _node_rows(node, step, master):
    g = torch.Generator().manual_seed(700 + 31 * node + step)
    return master + torch.randn(master.numel(), generator=g) * 1e-3


def _start():
    return torch.randn(N, generator=torch.Generator().manual_seed(3)) * 0.02


def _gloo_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    import fake_outer_adam_ops
    fake_outer_adam_ops.install()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gym_amd.comm import Collective
        from gym_amd.engine import DiLoCoOuterAdam
        out = {}
        for tag, kw in (("allreduce", dict(shard=False)), ("shard", dict(shard=True, chunks=2))):
            eng = DiLoCoOuterAdam(Collective(), 1, N, "cpu", torch.float32, **HP, **kw)
            per = N // world if kw["shard"] else N
            assert eng.shard is kw["shard"] and eng.per == per and eng._state.numel() == 3 * per
            assert eng.master.numel() == eng.exp_avg.numel() == eng.exp_avg_sq.numel() == per
            if kw["shard"]:
                assert len(eng.plan.bounds) == 2 and eng.rs_out.numel() == per and eng.sum is None
            eng.init_master(_start())
            x = _start().view(1, -1)
            for step in range(1, STEPS + 1):
                x = _node_rows(rank, step, x[0]).view(1, -1)
                eng(x)
                assert eng.t == step and sum(eng.launch_elems) == per
            out[f"{tag}_x"] = x[0].numpy()
            # the whole master / moments in arena order, from every rank's shard
            for name, part in (("p", eng.master), ("m", eng.exp_avg), ("v", eng.exp_avg_sq)):
                out[f"{tag}_{name}"] = part.numpy()
            if kw["shard"]:
                out["own"] = np.asarray(eng.plan.own)
        np.savez(os.path.join(out_dir, f"g{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_gloo_processes_match_two_replicas(tmp_path, fake):
    """World 2 x 1 node over gloo, all-reduce branch and sharded plan (state 1 /
    world per rank), against 2 replicas in one process: a sum of two is
    order-free, so every rank's parameters and state are bit-identical."""
    import torch.multiprocessing as mp
    from strategy_scenarios import free_port
    from gym_amd.engine import DiLoCoOuterAdam
    mp.spawn(_gloo_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    res = [dict(np.load(tmp_path / f"g{r}.npz")) for r in range(2)]
    eng = DiLoCoOuterAdam(Local(), 2, N, "cpu", torch.float32, **HP)
    eng.init_master(_start())
    reps = torch.stack([_start(), _start()])
    for step in range(1, STEPS + 1):
        reps = torch.stack([_node_rows(k, step, reps[k]) for k in range(2)])
        eng(reps)
    want = dict(x=reps[0].numpy(), p=eng.master.numpy(), m=eng.exp_avg.numpy(), v=eng.exp_avg_sq.numpy())
    assert fake.CALLS == [("plain", N, 0)] * STEPS
    for r in range(2):
        for name in ("x", "p", "m", "v"):
            assert np.array_equal(res[r][f"allreduce_{name}"], want[name]), (r, name)
        assert np.array_equal(res[r]["shard_x"], want["x"])
        own = np.concatenate([np.arange(a, b) for a, b in res[r]["own"]])
        assert len(own) == N // 2
        for name in ("p", "m", "v"):
            assert np.array_equal(res[r][f"shard_{name}"], want[name][own]), (r, name)
    assert not np.array_equal(want["x"], _start().numpy()) and want["v"].any()


# -------------------------------------------------------------- strategies --
def _init_diloco(**kw):
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    torch.manual_seed(42)
    model = R._model("x", torch.device("cpu"))
    s = DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.SGD, lr=0.05), H=2, **kw)
    s._init_node(model, 0, 1)
    return s, model


def test_diloco_strategy_takes_the_engine(fake):
    from gym_amd.engine import DiLoCoOuter, DiLoCoOuterAdam
    from gym_amd.strategy import OptimSpec
    adam = OptimSpec(torch.optim.Adam, lr=0.05)
    s, model = _init_diloco(outer_optim_spec=adam)
    assert isinstance(s.engine, DiLoCoOuterAdam) and s.outer_optimizer is None
    assert s.engine.hp == dict(lr=0.05, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False)
    for t in range(3):
        s.zero_grad()
        R._set_grads(model, 0, t, torch.device("cpu"))
        s.step()
    assert s.engine.t == 1 and fake.CALLS == [("plain", s.arena.n, 0)]
    s, _ = _init_diloco(outer_optim_spec=OptimSpec(torch.optim.AdamW, lr=0.05, weight_decay=0.1))
    assert isinstance(s.engine, DiLoCoOuterAdam) and s.engine.hp["decoupled"] and s.engine.hp["weight_decay"] == 0.1
    for kw in (dict(outer_optim_spec=adam, fused_outer=False),
               dict(outer_optim_spec=OptimSpec(torch.optim.Adam, lr=0.05, amsgrad=True))):
        s, _ = _init_diloco(**kw)
        assert s.engine is None and isinstance(s.outer_optimizer, torch.optim.Adam)
    s, _ = _init_diloco(fused_outer=False)  # no effect on an SGD spec
    assert type(s.engine) is DiLoCoOuter and s.outer_optimizer is None


def test_sparta_diloco_branches_with_the_adam_engine(fake):
    """Which launch a boundary step takes with an Adam outer optimizer: the
    masked one-pass step when fused, the sparse average then the plain step when
    not (bit-identical), torch's optimizer with fused_outer=False."""
    from gym_amd.engine import DiLoCoOuterAdam
    fused, s1, g1 = SD.run_replica_mode("sparta_diloco", 3, "cpu", True, outer_optim="adam")
    assert s1.fuse_boundary is True and isinstance(s1.engine, DiLoCoOuterAdam) and s1.engine.t == 2
    assert [c[0] for c in fake.CALLS] == ["masked", "masked"] and all(c[2] > 0 for c in fake.CALLS)
    del fake.CALLS[:]
    plain, s2, g2 = SD.run_replica_mode("sparta_diloco", 3, "cpu", True, outer_optim="adam", fuse_boundary=False)
    assert s2.fuse_boundary is False and isinstance(s2.engine, DiLoCoOuterAdam)
    assert [c[0] for c in fake.CALLS] == ["plain", "plain"]
    R.compare(plain, fused, rtol=0, atol=0)
    assert np.array_equal(g1, g2)
    del fake.CALLS[:]
    torch_run, s3, _ = SD.run_replica_mode("sparta_diloco", 3, "cpu", True, outer_optim="adam", fused_outer=False)
    assert s3.fuse_boundary is False and fake.CALLS == [] and getattr(s3, "engine", None) is None
    assert all(np.isfinite(x).all() for node in torch_run for x in node)


# ------------------------------------------------------------- ABI, no GPU --
_P = ctypes.c_void_p(64)
_Q = ctypes.c_void_p(128)
_SC = (0.1, 0.999, 0.001, 1e-8, 1.0, 0.0, -0.5, 0.03)


def _plain(L, src=_P, K=2, ld=8, n=8, div=2.0, master=_P, m=_P, v=_P, dst=_P, K_out=2, ld_dst=8, dtype=0):
    return L.ga_diloco_outer_adam(dtype, src, K, ld, n, div, master, m, v, *_SC, dst, K_out, ld_dst, None)


def _masked(L, src=_P, K=2, ld=8, n=8, bits=_P, sd=2.0, div=2.0, master=_P, m=_P, v=_P, dst=_P, K_out=2, ld_dst=8,
            dtype=0):
    return L.ga_diloco_outer_adam_masked(dtype, src, K, ld, n, bits, sd, div, master, m, v, *_SC, dst, K_out, ld_dst,
                                         None)


@pytest.mark.parametrize("bad", [
    dict(src=None), dict(master=None), dict(m=None), dict(v=None), dict(dst=None),
    dict(ld=4), dict(ld_dst=4), dict(div=0.0), dict(n=-1), dict(K=0), dict(K_out=-1), dict(dtype=7),
])
def test_outer_adam_invalid_arguments_fail_cleanly(bad):
    from gym_amd import _lib
    L = _lib.lib()
    assert _plain(L, **bad) == 1  # GA_EINVAL, checked on the host before any launch
    assert "ga_diloco_outer_adam" in L.ga_last_error().decode()


@pytest.mark.parametrize("bad", [
    dict(dst=_Q), dict(K_out=1), dict(K_out=0, dst=None), dict(ld_dst=16), dict(bits=None), dict(sd=0.0),
    dict(sd=-2.0), dict(div=0.0), dict(src=None, dst=None), dict(master=None), dict(m=None), dict(v=None),
    dict(ld=4, ld_dst=4), dict(n=-1), dict(K=0, K_out=0), dict(dtype=7),
])
def test_masked_outer_adam_invalid_arguments_fail_cleanly(bad):
    from gym_amd import _lib
    L = _lib.lib()
    assert _masked(L, **bad) == 1
    assert "ga_diloco_outer_adam_masked" in L.ga_last_error().decode()


def test_outer_adam_zero_length_is_a_noop():
    from gym_amd import _lib
    L = _lib.lib()
    assert _plain(L, n=0, src=None, dst=None, master=None, m=None, v=None) == 0
    assert L.ga_last_error().decode() == ""
    assert _masked(L, n=0, src=None, dst=None, bits=None, master=None, m=None, v=None) == 0
    assert _masked(L, n=0, sd=0.0) == 1  # ...but not a licence for a bad divisor
