"""The detailed node-drift metric without a GPU: ga_replica_gram_centered's argument
checks, the host algebra of gym_amd.metrics.drift_detail_summary against
np.corrcoef on close and far nodes, a float32 emulation of the kernel's summation
order against the error bound the GPU test asserts, NodeDrift's two paths over numpy
stand-ins, and the run log's two extra metrics."""
import ctypes
import json
import types

import numpy as np
import pytest
import torch

import drift_bounds
import fake_drift_ops
import fake_metrics_ops
from gym_amd import _lib

_P = ctypes.c_void_p(256)  # a non-null, aligned address no check dereferences
CLASSIC = {"correlation", "avg_model_correlation", "norm", "dist_to_mean", "consensus_distance"}
DETAIL = CLASSIC | {"one_minus_correlation", "avg_model_decorrelation", "pairwise_distance",
                    "max_pairwise_distance"}


@pytest.fixture(autouse=True)
def _keep_metrics_ops():
    """fake_drift_ops.install() is for a process of its own: put the real ops back."""
    import gym_amd.metrics as metrics
    real = metrics.ops
    yield
    metrics.ops = real


# ---- ABI ------------------------------------------------------------------------

def _centered(L, dtype=0, src=_P, K=2, ld=8, n=8, cgram=_P, mdot=_P, dsum=_P, mstat=_P, work=_P):
    return L.ga_replica_gram_centered(dtype, src, K, ld, n, cgram, mdot, dsum, mstat, work, None)


@pytest.mark.parametrize("kw", [dict(src=None), dict(cgram=None), dict(mdot=None), dict(dsum=None), dict(mstat=None),
                                dict(work=None), dict(K=0), dict(K=2, ld=4, n=8), dict(dtype=7)],
                         ids=["null-src", "null-cgram", "null-mdot", "null-dsum", "null-mstat", "null-work", "K=0",
                              "ld<n", "dtype"])
def test_invalid_arguments_fail_cleanly(kw):
    L = _lib.lib()
    assert _centered(L, **kw) == 1  # GA_EINVAL, on the host before any launch
    assert L.ga_last_error().decode()


def test_more_than_32_replicas_is_unsupported():
    L = _lib.lib()
    assert _centered(L, K=33, ld=8, n=8) == 3  # GA_EUNSUP
    assert "33" in L.ga_last_error().decode()
    assert L.ga_replica_gram_centered_workspace_bytes(33, 8) == -1
    assert L.ga_replica_gram_centered_workspace_bytes(0, 8) == -1
    assert L.ga_replica_gram_centered_workspace_bytes(2, -1) == -1


def test_workspace_is_one_partial_per_16384_columns():
    L = _lib.lib()
    for K in (1, 8, 17, 32):
        assert L.ga_replica_gram_centered_workspace_bytes(K, 0) == 0
        per = (K * K + 2 * K + 2) * 4
        for n in (1, 16384, 16385, 200003, 124_000_000):
            assert L.ga_replica_gram_centered_workspace_bytes(K, n) == -(-n // 16384) * per, (K, n)


def test_zero_length_returns_ok():
    L = _lib.lib()
    assert L.ga_replica_gram_centered(0, None, 2, 0, 0, None, None, None, None, None, None) == 0
    assert L.ga_last_error().decode() == ""


def test_op_refuses_cpu_tensors():
    from gym_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.replica_gram_centered(torch.zeros(2, 64))


# ---- host algebra ------------------------------------------------------------------

def _close_rows(K, delta, n=1000):
    rng = np.random.default_rng(10 * K + 1)
    base = rng.standard_normal((1, n)) + 0.5
    return base + delta * rng.standard_normal((K, n))


@pytest.mark.parametrize("delta", [1.0, 1e-3, 1e-6])
@pytest.mark.parametrize("K", [2, 5])
def test_detail_matches_corrcoef_and_the_classic_summary(K, delta):
    from gym_amd.metrics import drift_detail_summary, drift_summary
    x = _close_rows(K, delta)
    n = x.shape[1]
    got = drift_detail_summary(*fake_drift_ops.reference(x), n)
    assert set(got) == DETAIL
    omc = np.array(got["one_minus_correlation"])
    off = ~np.eye(K, dtype=bool)
    want = drift_bounds.one_minus_corr(x)
    print(f"K={K} delta={delta}: 1 - corr ~ {want[off].mean():.3g}, max relative error "
          f"{np.max(np.abs(omc - want)[off] / want[off]):.3g}")
    np.testing.assert_allclose(omc[off], want[off], rtol=1e-9, atol=0)
    # np.corrcoef itself, to the digits float64 leaves of 1 - corr
    np.testing.assert_allclose(omc[off], (1.0 - np.corrcoef(x))[off], rtol=1e-9, atol=8 * np.finfo(np.float64).eps)
    assert np.all(np.abs(np.diag(omc)) <= 1e-15)
    iu = np.triu_indices(K, k=1)
    assert abs(got["avg_model_decorrelation"] - omc[iu].mean()) <= 1e-15 * omc[iu].mean()
    pair = np.array(got["pairwise_distance"])
    want_pair = drift_bounds.pairwise_distance(x)
    np.testing.assert_allclose(pair, want_pair, rtol=1e-9, atol=0)
    assert got["max_pairwise_distance"] == pair[iu].max()
    # today's five keys
    classic = drift_summary(*fake_metrics_ops.reference(x), n)
    for key in ("norm", "dist_to_mean", "consensus_distance"):
        np.testing.assert_allclose(got[key], classic[key], rtol=1e-12, atol=0, err_msg=key)
    if delta == 1e-6:
        # the classic correlation has lost 1 - corr ~ 1e-12 to its own rounding: compare loosely
        np.testing.assert_allclose(1.0 - np.array(got["correlation"]), 1.0 - np.array(classic["correlation"]),
                                   rtol=0, atol=1e-10)
        assert abs(got["avg_model_correlation"] - classic["avg_model_correlation"]) <= 1e-10
    else:
        np.testing.assert_allclose(got["correlation"], classic["correlation"], rtol=0, atol=1e-12)
        assert abs(got["avg_model_correlation"] - classic["avg_model_correlation"]) <= 1e-12
    # zero padding beyond the real elements changes nothing
    xp = np.concatenate([x, np.zeros((K, 24))], axis=1)
    padded = drift_detail_summary(*fake_drift_ops.reference(xp), n)
    for key in DETAIL:
        np.testing.assert_allclose(padded[key], got[key], rtol=1e-12, atol=1e-15, err_msg=key)


def test_reconstructs_gram_and_rowsum():
    x = _close_rows(5, 1e-3)
    C, b, t, (A, S) = fake_drift_ops.reference(x)
    G, s, d2 = fake_metrics_ops.reference(x)
    np.testing.assert_allclose(A + b[:, None] + b[None, :] + C, G, rtol=1e-12)
    np.testing.assert_allclose(S + t, s, rtol=1e-12)
    np.testing.assert_allclose(np.diag(C), d2, rtol=1e-12)


def test_zero_variance_row_is_nan_like_corrcoef():
    from gym_amd.metrics import drift_detail_summary
    x = np.random.default_rng(0).standard_normal((3, 100))
    x[1] = 2.0
    got = drift_detail_summary(*fake_drift_ops.reference(x), 100)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.corrcoef(x)
    for key, ref in (("one_minus_correlation", 1.0 - want), ("correlation", want)):
        g = np.array(got[key])
        assert np.array_equal(np.isnan(g), np.isnan(ref)), key
        assert np.isnan(g[1]).all() and np.isnan(g[:, 1]).all()
        assert abs(g[0, 2] - ref[0, 2]) < 1e-12
    assert np.isfinite(got["pairwise_distance"]).all()


def test_identical_rows_are_at_distance_zero():
    from gym_amd.metrics import drift_detail_summary
    x = _close_rows(4, 1e-3)
    x[3] = x[1]
    got = drift_detail_summary(*fake_drift_ops.reference(x), x.shape[1])
    pair, omc = np.array(got["pairwise_distance"]), np.array(got["one_minus_correlation"])
    assert pair[1, 3] == 0.0 and pair[3, 1] == 0.0
    assert 0.0 <= omc[1, 3] <= 1e-15 and 0.0 <= omc[3, 1] <= 1e-15
    assert pair[0, 1] > 0.0 and omc[0, 1] > 0.0


# ---- the kernel's arithmetic in float32, against the GPU test's bound ----------------

@pytest.mark.parametrize("K", [8, 32])
def test_float32_emulation_stays_inside_the_bound(K):
    """drift_bounds.emulate follows the kernel's order (ascending-k mean, true
    division, fp32 d, fma chains of at most L per accumulator, fp32 combines, fp64
    final sum); its distance from float64 must sit inside the first-order bound the
    GPU test holds the kernel to, with room to spare."""
    L = _lib.lib().ga_replica_gram_chain()
    x = torch.randn(K, 20011, generator=torch.Generator().manual_seed(100 + K)).numpy()
    got = drift_bounds.emulate(x, L)
    ref, bound = drift_bounds.reference_and_bounds(x, L)
    for name, g, r, bd in zip(("cgram", "mdot", "dsum", "mstat"), got, ref, bound):
        ratio = np.max(np.abs(g - r) / bd)
        print(f"K={K} {name}: emulation max err/bound {ratio:.3g}")
        assert ratio <= 1.0, name


# ---- NodeDrift -----------------------------------------------------------------------

class _World:
    def __init__(self, world):
        self.world, self.rank, self.exchange = world, 0, world > 1


def _rows(K=4, ld=96, n=80, n_true=77):
    g = torch.Generator().manual_seed(3)
    P = torch.randn(K, ld, generator=g)
    P[:, n_true:n] = 0.0
    P[:, n:] = 1e30
    return P, ld, n, n_true


def test_default_is_todays_path_and_never_touches_the_centred_kernel():
    from gym_amd.metrics import NodeDrift, drift_summary
    P, ld, n, n_true = _rows()
    fake_drift_ops.install(centered=False)
    out = NodeDrift(_World(1), 4, ld, n, n_true, torch.device("cpu"), torch.float32)(P)
    assert set(out) == CLASSIC
    assert out == drift_summary(*fake_metrics_ops.reference(P[:, :n].double().numpy()), n_true)
    out = NodeDrift(_World(1), 4, ld, n, n_true, torch.device("cpu"), torch.float32, detail=False)(P)
    assert set(out) == CLASSIC


def test_detail_never_touches_the_plain_kernel():
    from gym_amd.metrics import NodeDrift, drift_detail_summary
    P, ld, n, n_true = _rows()
    fake_drift_ops.install(plain=False)
    out = NodeDrift(_World(1), 4, ld, n, n_true, torch.device("cpu"), torch.float32, detail=True)(P)
    assert set(out) == DETAIL
    assert out == drift_detail_summary(*fake_drift_ops.reference(P[:, :n].double().numpy()), n_true)


@pytest.mark.parametrize("K_local", [1, 2])
def test_node_drift_detail_over_gloo(tmp_path, K_local):
    """World of 3, K_local rows each: rank 0's nine keys equal numpy's on the same
    per-rank seeded vectors in node order, the other ranks get None."""
    import torch.multiprocessing as mp
    from strategy_scenarios import free_port
    world, ld, n, n_true = 3, 1024, 1000, 990
    mp.spawn(fake_drift_ops.drift_worker, args=(world, free_port(), K_local, ld, n, n_true, str(tmp_path)),
             nprocs=world, join=True)
    res = [json.load(open(tmp_path / f"r{r}.json")) for r in range(world)]
    assert res[1] is None and res[2] is None
    x = torch.cat([fake_metrics_ops.rank_rows(r, K_local, ld, n, n_true) for r in range(world)])
    x = x[:, :n_true].double().numpy()
    N = world * K_local
    got = res[0]
    assert set(got) == DETAIL
    iu = np.triu_indices(N, k=1)
    corr = np.corrcoef(x)
    np.testing.assert_allclose(np.array(got["correlation"]), corr, rtol=0, atol=1e-12)
    assert abs(got["avg_model_correlation"] - corr[iu].mean()) < 1e-12
    np.testing.assert_allclose(got["norm"], np.linalg.norm(x, axis=1), rtol=1e-12)
    d = np.linalg.norm(x - x.mean(axis=0), axis=1)
    np.testing.assert_allclose(got["dist_to_mean"], d, rtol=1e-12)
    np.testing.assert_allclose(got["consensus_distance"], (d * d).mean(), rtol=1e-12)
    omc = drift_bounds.one_minus_corr(x)
    off = ~np.eye(N, dtype=bool)
    np.testing.assert_allclose(np.array(got["one_minus_correlation"])[off], omc[off], rtol=1e-9)
    np.testing.assert_allclose(got["avg_model_decorrelation"], omc[iu].mean(), rtol=1e-9)
    pair = drift_bounds.pairwise_distance(x)
    np.testing.assert_allclose(got["pairwise_distance"], pair, rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["max_pairwise_distance"], pair.max(), rtol=1e-9)


# ---- run log ---------------------------------------------------------------------------

def _run_log():
    from gym_amd.strategy import OptimSpec, SimpleReduceStrategy
    from gym_amd.train_node import RunLog
    return RunLog(SimpleReduceStrategy(optim_spec=OptimSpec(torch.optim.SGD, lr=0.1)), 6)


def _replica_node(detail):
    """What ReplicaTrainNode._node_drift reads of a node: 4 rows of one process."""
    P, ld, n, n_true = _rows(ld=96, n=96, n_true=90)
    P[:, n_true:] = 0.0
    ra = types.SimpleNamespace(ld=ld, layout=types.SimpleNamespace(n_params=n_true), device=torch.device("cpu"),
                               dtype=torch.float32, flat_set=P)
    return types.SimpleNamespace(runner=types.SimpleNamespace(ra=ra, coll=_World(1)), K=4, drift=None,
                                 drift_detail=detail, logger=_run_log())


class _TwoNodes:
    """A Collective of two nodes for rank 0: the other node's arena is this one's + 1e-3."""
    world, rank, exchange = 2, 0, True

    def all_gather_into(self, full, shard):
        full.view(2, -1)[0].copy_(shard)
        full.view(2, -1)[1].copy_(shard + 1e-3 * torch.arange(shard.numel()) / shard.numel())


def _train_node(detail, monkeypatch):
    """What TrainNode._node_drift reads of a node whose strategy has no arena."""
    import gym_amd.comm as comm
    import tiny_models
    monkeypatch.setattr(comm, "Collective", _TwoNodes)
    torch.manual_seed(0)
    return types.SimpleNamespace(strategy=object(), model=tiny_models.TinyMLP(), rank=0, drift=None,
                                 drift_detail=detail, logger=_run_log())


@pytest.mark.parametrize("detail", [False, True])
@pytest.mark.parametrize("kind", ["replica", "process"])
def test_run_log_takes_the_two_new_metrics_only_with_the_flag(kind, detail, monkeypatch):
    from gym_amd.replica import ReplicaTrainNode
    from gym_amd.train_node import TrainNode
    fake_drift_ops.install(plain=not detail, centered=detail)
    if kind == "replica":
        node, measure = _replica_node(detail), ReplicaTrainNode._node_drift
    else:
        node, measure = _train_node(detail, monkeypatch), TrainNode._node_drift
    for step in range(1, 7):
        node.logger.increment_step()
        if step % 3 == 0:
            out = measure(node)
            assert set(out) == (DETAIL if detail else CLASSIC)
    names = ["avg_model_correlation", "consensus_distance"]
    if detail:
        names += ["avg_model_decorrelation", "max_pairwise_distance"]
    got = node.logger.summary()["metrics"]
    assert [(s, name) for s, name, _ in got] == [(s, name) for s in (3, 6) for name in names]
    assert all(np.isfinite(v) for _, _, v in got)
    if detail:
        assert dict(((s, nm), v) for s, nm, v in got)[(3, "max_pairwise_distance")] > 0.0


def test_nodes_take_the_flag_and_default_it_off():
    import inspect

    from gym_amd.replica import ReplicaTrainNode
    from gym_amd.train_node import TrainNode
    for cls in (TrainNode, ReplicaTrainNode):
        assert inspect.signature(cls.__init__).parameters["drift_detail"].default is False
