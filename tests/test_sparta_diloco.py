"""SPARTADiLoCoStrategy / DiLoCoCommunicator without a GPU: the import surface,
the host orchestration over gloo with the oracle-backed kernel stand-ins
(tests/fake_sparta_diloco_ops.py), and ga_diloco_outer_masked's argument
checks.  The kernel's arithmetic and the device runs: test_gpu_sparta_diloco.py."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import replica_scenarios as R
import sparta_diloco_scenarios as SD


@pytest.fixture
def fake(monkeypatch):
    import fake_ops
    import fake_sparta_diloco_ops as fsd
    import gym_amd.engine as engine
    import gym_amd.fused_optim as fused_optim
    import gym_amd.replica as replica
    import gym_amd.strategy.diloco as diloco
    import gym_amd.strategy.strategy as strategy
    for mod in (engine, diloco, fused_optim, replica):
        monkeypatch.setattr(mod, "ops", fake_ops)
    monkeypatch.setattr(fake_ops, "diloco_outer_masked", fsd.diloco_outer_masked, raising=False)
    monkeypatch.setattr(strategy, "require_gpu", lambda device: None)
    monkeypatch.setattr(fsd, "CALLS", [])
    return fsd


# ------------------------------------------------------------------ surface --
def test_import_surface():
    import exogym.strategy as es
    import gym_amd.strategy as gs
    from exogym.strategy import DiLoCoCommunicator, SPARTADiLoCoStrategy  # noqa: F401
    from exogym.strategy.diloco import DiLoCoCommunicator as C2
    from exogym.strategy.sparta_diloco import SPARTADiLoCoStrategy as S2  # the example's import (nanogpt.py:224)
    import exogym.strategy.sparta_diloco as shim
    import gym_amd.strategy.sparta_diloco as impl
    assert shim is impl
    assert S2 is gs.SPARTADiLoCoStrategy is es.SPARTADiLoCoStrategy
    assert C2 is gs.DiLoCoCommunicator is es.DiLoCoCommunicator is gs.diloco.DiLoCoCommunicator
    for name in ("SPARTADiLoCoStrategy", "DiLoCoCommunicator"):
        assert name in gs.__all__ and name in es.__all__
    ns = {}
    exec("from exogym.strategy import *", ns)  # raises AttributeError in the reference (its __all__ names the class)
    assert ns["SPARTADiLoCoStrategy"] is S2


def test_construction_and_class_layout():
    from gym_amd.strategy import (CommunicateOptimizeStrategy, DiLoCoCommunicator, DiLoCoStrategy, OptimSpec,
                                  SPARTADiLoCoStrategy, SPARTAStrategy)
    from gym_amd.strategy.sparta import RandomIndexSelector, SparseCommunicator
    s = SPARTADiLoCoStrategy()
    assert isinstance(s, CommunicateOptimizeStrategy) and not isinstance(s, (SPARTAStrategy, DiLoCoStrategy))
    sp, dl = s.communication_modules
    assert type(sp) is SparseCommunicator and type(dl) is DiLoCoCommunicator
    assert type(sp.index_selector) is RandomIndexSelector and s.index_selector is sp.index_selector
    assert (s.index_selector.p, s.index_selector.mask_source, dl.H) == (0.005, "torch", 100)
    assert s.inner_optim_spec.cls is torch.optim.AdamW
    want = DiLoCoStrategy().outer_optim_spec
    assert (dl.outer_optim_spec.cls, dl.outer_optim_spec.kwargs) == (want.cls, want.kwargs)
    assert want.cls is torch.optim.SGD and want.kwargs == dict(lr=0.7, nesterov=True, momentum=0.9)
    c = DiLoCoCommunicator()
    assert c.H == 100 and c.outer_optim_spec.kwargs == want.kwargs
    s = SPARTADiLoCoStrategy(inner_optim="sgd", outer_optim=OptimSpec(torch.optim.Adam, lr=0.1), p_sparta=0.25, H=7,
                             mask_source="philox", placement=False)
    assert s.inner_optim_spec.cls is torch.optim.SGD and s.outer_optim_spec.cls is torch.optim.Adam
    assert s.communication_modules[1].H == 7 and s.index_selector.mask_source == "philox"
    assert s.placement_opt is False and s.fuse_boundary is False  # Philox keeps no mask in memory


def test_example_call_and_pickling():
    """example/nanogpt.py:233-242 passes inner_optim_spec= / outer_optim_spec= /
    sparta_interval=, which the constructor does not know: kept, not used (Q5)."""
    from exogym.strategy import OptimSpec
    from exogym.strategy.sparta_diloco import SPARTADiLoCoStrategy
    inner = OptimSpec(torch.optim.AdamW, lr=3e-4)
    outer = OptimSpec(torch.optim.SGD, lr=0.5, nesterov=False, momentum=0.8)
    s = SPARTADiLoCoStrategy(inner_optim_spec=inner, outer_optim_spec=outer, H=50, p_sparta=0.01, sparta_interval=3,
                             lr_scheduler="lambda_cosine", lr_scheduler_kwargs={"warmup_steps": 10}, max_norm=1.0)
    assert s.kwargs["inner_optim_spec"] is inner and s.kwargs["outer_optim_spec"] is outer
    assert s.sparta_interval == 3 and s.H == 50 and s.p_sparta == 0.01 and s.max_norm == 1.0
    # ... and the optimizers are the defaults, as the unknown keywords are ignored
    assert s.inner_optim_spec.kwargs == {} and s.outer_optim_spec.kwargs == dict(lr=0.7, nesterov=True, momentum=0.9)
    s2 = pickle.loads(pickle.dumps(s))  # strategies cross mp.spawn by pickle before _init_node
    assert (s2.H, s2.p_sparta, s2.sparta_interval, s2.lr_scheduler) == (50, 0.01, 3, "lambda_cosine")
    assert s2.communication_modules[0].strategy is s2 and s2.communication_modules[1].H == 50
    cfg = s.__config__()
    assert cfg["strategy"] == "SPARTADiLoCoStrategy"
    assert (cfg["H"], cfg["p_sparta"], cfg["fuse_boundary"], cfg["mask_draw"]) == (50, 0.01, True, None)
    assert cfg["placement"] == {"enabled": True, "records": {}}


def test_bad_optimizers_raise():
    from gym_amd.strategy import DiLoCoCommunicator, SPARTADiLoCoStrategy
    with pytest.raises(ValueError, match="Unknown optimizer"):
        SPARTADiLoCoStrategy(inner_optim="lion")
    with pytest.raises(ValueError, match="Unknown optimizer"):
        SPARTADiLoCoStrategy(outer_optim="lion")
    with pytest.raises(TypeError, match="Expected str, OptimSpec, or None"):
        SPARTADiLoCoStrategy(inner_optim=torch.optim.SGD)
    with pytest.raises(TypeError, match="Expected str, OptimSpec, or None"):
        DiLoCoCommunicator(outer_optim=3)
    with pytest.raises(ValueError, match="mask_source"):
        SPARTADiLoCoStrategy(mask_source="numpy")


def test_replica_layout_accepts_the_strategy():
    from gym_amd.replica import ReplicaRunner, replica_layout
    from gym_amd.strategy import SPARTADiLoCoStrategy
    assert ReplicaRunner.supports(SPARTADiLoCoStrategy())
    assert replica_layout(8, [0], "auto", SPARTADiLoCoStrategy()) == (1, 8)
    assert replica_layout(8, [0, 1], 4, SPARTADiLoCoStrategy(mask_source="philox", outer_optim="adam")) == (2, 4)


# ---------------------------------------------------- process per node, gloo --
@pytest.mark.parametrize("world", [2, 3])
def test_degenerate_identities(tmp_path, world):
    """With no outer step in the run the strategy is SPARTAStrategy; with
    nothing selected it is DiLoCoStrategy: same arguments and seed, same bits."""
    runs = [("combo_noH", dict(H=1000)), ("sparta", dict(kind="sparta")),
            ("combo_p0", dict(p_sparta=0.0)), ("diloco", dict(kind="diloco"))]
    res = SD.run_process_mode("sparta_diloco", world, "cpu", True, str(tmp_path), runs)
    R.compare(res["sparta"], res["combo_noH"], rtol=0, atol=0)
    R.compare(res["diloco"], res["combo_p0"], rtol=0, atol=0)
    for a, b in zip(res["sparta"][0], res["diloco"][0]):  # ...and the two baselines are different runs
        assert not np.array_equal(a, b)


@pytest.fixture(scope="module")
def process_runs(tmp_path_factory):
    """3 processes over gloo, once per scenario for the tests that compare against it."""
    cache = {}

    def get(name):
        if name not in cache:
            d = tmp_path_factory.mktemp(name)
            cache[name] = SD.run_process_mode(name, 3, "cpu", True, str(d))["run"]
        return cache[name]
    return get


@pytest.mark.parametrize("name", ["sparta_diloco", "sparta_diloco_frozen"])
def test_mixed_run_matches_the_restatement(process_runs, name):
    """H = 2, 5 steps, p = 0.1, AdamW inner, default outer, max_norm = 1: both
    modules fire at steps 2 and 4.  Differences: gloo's ring order against the
    ascending sum (compare's own tolerances)."""
    want = SD.restated(name, 3)
    R.compare(want, process_runs(name))
    for a, b in zip(want[0], want[2]):  # the last step is an outer step: every node holds the master
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", SD.NAMES)
def test_replicas_match_process_per_node(process_runs, fake, name):
    rep, s, _ = SD.run_replica_mode(name, 3, "cpu", True)
    R.compare(process_runs(name), rep)
    philox = name == "sparta_diloco_philox"
    assert s.fuse_boundary is (not philox) and s.mask_draw == ("philox" if philox else "torch")
    assert len(fake.CALLS) == (0 if philox else 2)  # local_step 2 and 4


@pytest.mark.parametrize("name", SD.NAMES)
def test_replica_processes_match_process_per_node(tmp_path, name):
    """2 processes x 2 local nodes (gloo) == 4 processes of one node: with an
    exchange the runner runs the two engines one after the other."""
    (tmp_path / "p").mkdir()
    (tmp_path / "r").mkdir()
    proc = SD.run_process_mode(name, 4, "cpu", True, str(tmp_path / "p"))["run"]
    rep = SD.run_replica_processes(name, 2, 2, "cpu", True, str(tmp_path / "r"))
    R.compare(proc, rep)


@pytest.mark.parametrize("name", ["sparta_diloco", "sparta_diloco_frozen"])
def test_fused_boundary_equals_two_launches(fake, name):
    fused, s1, g1 = SD.run_replica_mode(name, 3, "cpu", True)
    n_fused = len(fake.CALLS)
    plain, s2, g2 = SD.run_replica_mode(name, 3, "cpu", True, fuse_boundary=False)
    assert s1.fuse_boundary is True and s2.fuse_boundary is False
    assert n_fused == 2 and len(fake.CALLS) == 2 and all(sel > 0 for _, sel in fake.CALLS)
    R.compare(plain, fused, rtol=0, atol=0)
    assert np.array_equal(g1, g2)  # the torch generator advanced the same way
    cfg = s1.__config__()
    assert cfg["fuse_boundary"] is True and cfg["mask_draw"] == "torch" and cfg["H"] == 2 and cfg["p_sparta"] == 0.1
    assert s2.__config__()["fuse_boundary"] is False


def test_other_selectors_and_generic_outer(fake):
    """A selector whose masks exist only as bytes is packed for the one-pass
    step; a non-SGD outer optimizer has no fused engine and keeps two launches."""
    from gym_amd.strategy.sparta import ShuffledSequentialIndexSelector

    def swap(s):
        sel = ShuffledSequentialIndexSelector(0.25)
        s.index_selector = s.communication_modules[0].index_selector = sel

    def run(**over):
        from gym_amd.replica import ReplicaRunner
        torch.manual_seed(42)
        models = [R._model("x", torch.device("cpu")) for _ in range(3)]
        s = SD.make_strategy("sparta_diloco", **over)
        if "outer_optim" not in over:
            swap(s)
        runner = ReplicaRunner(s, models, rank=0, num_nodes=3)
        for t in range(SD.STEPS):
            runner.zero_grad()
            for k, m in enumerate(models):
                R._set_grads(m, k, t, torch.device("cpu"))
            runner.step()
        return [SD._host_params(m) for m in models], s

    a, sa = run()
    assert sa.fuse_boundary is True and len(fake.CALLS) == 2
    b, sb = run(fuse_boundary=False)
    R.compare(b, a, rtol=0, atol=0)
    c, sc = run(outer_optim="adam")
    assert sc.fuse_boundary is False and len(fake.CALLS) == 2
    assert all(np.isfinite(x).all() for node in c for x in node)


def _hand_built_worker(rank, world, port, out_dir):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    SD._install(True)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gym_amd.strategy import CommunicateOptimizeStrategy, DiLoCoCommunicator, OptimSpec
        from gym_amd.strategy.federated_averaging import AveragingCommunicator
        from gym_amd.strategy.sparta import PartitionedIndexSelector, SparseCommunicator
        out = {}
        for tag, first in (("avg", lambda: AveragingCommunicator()),
                           ("sparse", lambda: SparseCommunicator(PartitionedIndexSelector(0.25)))):
            torch.manual_seed(42)
            model = R._model("x", torch.device("cpu"))
            s = CommunicateOptimizeStrategy([first(), DiLoCoCommunicator(H=2)],
                                            inner_optim=OptimSpec(torch.optim.SGD, lr=0.05))
            s._init_node(model, rank, world)
            for t in range(3):
                s.zero_grad()
                R._set_grads(model, rank, t, torch.device("cpu"))
                s.step()
            s.finish()
            out.update({f"{tag}_{i}": p for i, p in enumerate(SD._host_params(model))})
            assert s.placement_records() == {}
        np.savez(os.path.join(out_dir, f"h{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_communicator_in_a_hand_built_strategy(tmp_path):
    """DiLoCoCommunicator behind another module in a CommunicateOptimizeStrategy
    built by hand: it runs, and after the outer step at local_step 2 (the last
    step) every node holds the master."""
    import torch.multiprocessing as mp
    from strategy_scenarios import free_port
    mp.spawn(_hand_built_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = (np.load(tmp_path / f"h{r}.npz") for r in range(2))
    start = [p.detach().numpy() for p in R._model("x", torch.device("cpu")).parameters()]
    for tag in ("avg", "sparse"):
        for i in range(len(R.SHAPES)):
            assert np.array_equal(a[f"{tag}_{i}"], b[f"{tag}_{i}"])
            assert not np.array_equal(a[f"{tag}_{i}"], start[i])


def test_masked_outer_needs_a_local_step(fake):
    from gym_amd.engine import DiLoCoOuter

    class Exchanging:
        world, rank, exchange, rccl, backend = 2, 0, True, False, "gloo"

    eng = DiLoCoOuter(Exchanging(), 1, 128, "cpu", torch.float32)
    with pytest.raises(ValueError, match="no-exchange"):
        eng(torch.zeros(1, 128), sparse_mask=torch.zeros(2, dtype=torch.int64))
    assert fake.CALLS == []


def test_generic_outer_takes_no_mask(fake):
    """torch's optimizer has no one-pass masked form: a sparse_mask is an error
    before anything is read or written."""
    from gym_amd.comm import Collective
    from gym_amd.engine import TorchOuter
    from gym_amd.strategy import OptimSpec
    eng = TorchOuter(Collective(), 2, 128, "cpu", torch.float32, OptimSpec(torch.optim.Adam, lr=0.1))
    rows = torch.ones(2, 128)
    eng.init_master(rows[0])
    with pytest.raises(ValueError, match="masked"):
        eng(rows, sparse_mask=torch.zeros(2, dtype=torch.int64))
    assert torch.equal(rows, torch.ones(2, 128)) and not eng.optimizer.state


# ------------------------------------------------------------- ABI, no GPU --
_P = ctypes.c_void_p(64)
_Q = ctypes.c_void_p(128)


def _masked(L, src=_P, K=2, ld=8, n=8, bits=_P, sd=2.0, div=2.0, master=_P, mom=_P, first=1, momentum=0.9, damp=0.0,
            nesterov=1, dst=_P, K_out=2, ld_dst=8, dtype=0, master_f32=1):
    return L.ga_diloco_outer_masked(dtype, src, K, ld, n, bits, sd, div, master, mom, master_f32, first, 0.7, momentum,
                                    damp, 0.0, nesterov, dst, K_out, ld_dst, None)


@pytest.mark.parametrize("bad", [
    dict(dst=_Q),               # not in place
    dict(K_out=1),              # a row SPARTA wrote would keep its average
    dict(K_out=0, dst=None),
    dict(ld_dst=16),
    dict(bits=None),            # null mask words with n > 0
    dict(sd=0.0), dict(sd=-2.0),
    dict(div=0.0),
    dict(src=None, dst=None), dict(master=None),
    dict(mom=None),             # momentum != 0 without a buffer
    dict(ld=4, ld_dst=4),       # rows overlap
    dict(n=-1), dict(K=0, K_out=0),
    dict(damp=0.1),             # Nesterov with dampening
    dict(dtype=1, master_f32=0),  # bf16 master
    dict(dtype=7),
])
def test_masked_outer_invalid_arguments_fail_cleanly(bad):
    from gym_amd import _lib
    L = _lib.lib()
    assert _masked(L, **bad) == 1  # GA_EINVAL, checked on the host before any launch
    assert "ga_diloco_outer_masked" in L.ga_last_error().decode()


def test_masked_outer_zero_length_is_a_noop():
    from gym_amd import _lib
    L = _lib.lib()
    assert _masked(L, n=0, src=None, dst=None, bits=None, master=None, mom=None) == 0
    assert L.ga_last_error().decode() == ""
    assert _masked(L, n=0, sd=0.0) == 1  # ...but not a licence for a bad divisor
