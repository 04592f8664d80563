"""The strategies with an Adam / AdamW outer optimizer on the MI355X: every outer
step of DiLoCoStrategy (one node) and of the replica runner (K = 3) checked from
the state read back before it against torch's optimizer loaded with that state
(tests/outer_adam_checks.py: one step at a time, never a trajectory), the
switches that keep torch's optimizer, and SPARTA+DiLoCo's one-pass boundary
step with the Adam engine against its two launches."""
import numpy as np
import pytest
import torch

import outer_adam_checks as C
import replica_scenarios as R
import sparta_diloco_scenarios as SD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS = 7  # H = 2: outer steps at local_step 2, 4, 6


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gym_amd import _lib
    _lib.lib()


@pytest.fixture(autouse=True)
def _real_kernel_layer(monkeypatch):
    """These tests run the product's kernels: a CPU stand-in that an earlier test of
    the same process left installed in the gym_amd modules is put aside for them."""
    import sys

    import gym_amd.ops as real
    import gym_amd.replica  # noqa: F401  (imports every module that binds `ops`)
    import gym_amd.strategy  # noqa: F401
    for name, mod in list(sys.modules.items()):
        if name.startswith("gym_amd") and getattr(mod, "ops", real) is not real:
            monkeypatch.setattr(mod, "ops", real)


SPECS = {"adam": (torch.optim.Adam, dict(lr=0.05)),
         "adamw": (torch.optim.AdamW, dict(lr=0.05, weight_decay=0.1, betas=(0.8, 0.99)))}


def _tap(eng, rows_of):
    """Wrap an engine: (rows, master, exp_avg, exp_avg_sq, t) before and after every call."""
    log = []

    def snap():
        torch.cuda.synchronize()
        return [rows_of().clone(), eng.master.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), eng.t]

    def check_all(cls, kw, K):
        from oracle.reduce import mean_reduce
        assert [pre[4] for pre, _ in log] == list(range(len(log)))
        for pre, post in log:
            n = eng.n
            avg = torch.from_numpy(mean_reduce(list(pre[0][:, :n].cpu().numpy()), divisor=K)).to(DEV)
            want = C.torch_step(cls, kw, pre[1], pre[2], pre[3], pre[4], avg)
            got = [x.cpu().numpy() for x in post[1:4]]
            print(f"outer step {post[4]}: bit-identical shares vs torch {C.bit_shares(got, want)}")
            C.assert_step(got, want, f"outer step {post[4]}")
            assert post[4] == pre[4] + 1
            for k in range(K):
                assert torch.equal(post[0][k, :n], post[1])
    return log, snap, check_all


@pytest.mark.parametrize("name", list(SPECS))
def test_diloco_strategy_one_node_each_outer_step_against_torch(name):
    from gym_amd.engine import DiLoCoOuterAdam
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    cls, kw = SPECS[name]
    torch.manual_seed(42)
    model = R._model("x", torch.device(DEV))
    s = DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), outer_optim_spec=OptimSpec(cls, **kw), H=2)
    s._init_node(model, 0, 1)
    assert isinstance(s.engine, DiLoCoOuterAdam) and s.outer_optimizer is None
    log, snap, check_all = _tap(s.engine, lambda: s.arena.flat.view(1, -1))
    inner = s._outer_step

    def outer_step():
        pre = snap()
        inner()
        log.append((pre, snap()))
    s._outer_step = outer_step
    for t in range(STEPS):
        s.zero_grad()
        R._set_grads(model, 0, t, torch.device(DEV))
        s.step()
    assert len(log) == 3 and s.engine.t == 3
    check_all(cls, kw, 1)
    assert s.placement_records()["engine"]["placed"] is False


@pytest.mark.parametrize("over", [dict(fused_outer=False), dict(amsgrad=True)], ids=["fused_outer-off", "amsgrad"])
def test_switches_that_keep_torch(over):
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    torch.manual_seed(42)
    model = R._model("x", torch.device(DEV))
    kw = dict(lr=0.05, **{k: v for k, v in over.items() if k == "amsgrad"})
    s = DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2),
                       outer_optim_spec=OptimSpec(torch.optim.Adam, **kw), H=2,
                       **{k: v for k, v in over.items() if k == "fused_outer"})
    s._init_node(model, 0, 1)
    assert s.engine is None and isinstance(s.outer_optimizer, torch.optim.Adam)
    for t in range(3):
        s.zero_grad()
        R._set_grads(model, 0, t, torch.device(DEV))
        s.step()
    assert int(s.outer_optimizer.state[s.master]["step"]) == 1


@pytest.mark.parametrize("name", list(SPECS))
def test_replica_runner_three_nodes_each_outer_step_against_torch(name):
    from gym_amd.engine import DiLoCoOuterAdam
    from gym_amd.replica import ReplicaRunner
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    cls, kw = SPECS[name]
    K = 3
    torch.manual_seed(42)
    dev = torch.device(DEV)
    models = [R._model("x", dev) for _ in range(K)]
    s = DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), outer_optim_spec=OptimSpec(cls, **kw), H=2)
    runner = ReplicaRunner(s, models, rank=0, num_nodes=K)
    eng = runner.outer
    assert isinstance(eng, DiLoCoOuterAdam) and runner.outer_optimizer is None
    log, snap, check_all = _tap(eng, lambda: runner.ra.flat_set)

    def outer(P):
        pre = snap()
        eng(P)
        log.append((pre, snap()))
    runner.outer = outer
    for t in range(STEPS):
        runner.zero_grad()
        for k, m in enumerate(models):
            R._set_grads(m, k, t, dev)
        runner.step()
    assert len(log) == 3
    check_all(cls, kw, K)
    rows = log[0][0][0]
    assert not torch.equal(rows[0], rows[1])  # the nodes had drifted apart before the first outer step


def test_sparta_diloco_adam_one_pass_boundary_equals_two_launches():
    from gym_amd.engine import DiLoCoOuterAdam
    fused, s1, g1 = SD.run_replica_mode("sparta_diloco", 3, DEV, outer_optim="adam")
    plain, s2, g2 = SD.run_replica_mode("sparta_diloco", 3, DEV, outer_optim="adam", fuse_boundary=False)
    assert s1.fuse_boundary is True and s2.fuse_boundary is False
    assert isinstance(s1.engine, DiLoCoOuterAdam) and isinstance(s2.engine, DiLoCoOuterAdam)
    assert s1.engine.t == s2.engine.t == 2 and s1.mask_draw == s2.mask_draw
    R.compare(plain, fused, rtol=0, atol=0)
    assert np.array_equal(g1, g2)
    start = [p.detach().cpu().numpy() for p in R._model("x", torch.device("cpu")).parameters()]
    assert not np.array_equal(fused[0][0], start[0])
