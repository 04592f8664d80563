"""Node-drift metric without a GPU: ga_replica_gram's argument checks, the
Gram -> Pearson correlation host math against np.corrcoef, and NodeDrift's
gather + rank-0 result over a gloo world with a numpy stand-in for the kernel."""
import ctypes
import json

import numpy as np
import pytest
import torch

import fake_metrics_ops
from gym_amd import _lib

_P = ctypes.c_void_p(256)  # a non-null, aligned address no check dereferences


def _gram(L, dtype=0, src=_P, K=2, ld=8, n=8, gram=_P, rowsum=_P, dist2=_P, work=_P):
    return L.ga_replica_gram(dtype, src, K, ld, n, gram, rowsum, dist2, work, None)


@pytest.mark.parametrize("kw", [dict(src=None), dict(K=0), dict(K=2, ld=4, n=8), dict(dtype=7)],
                         ids=["null-src", "K=0", "ld<n", "dtype"])
def test_invalid_arguments_fail_cleanly(kw):
    L = _lib.lib()
    assert _gram(L, **kw) == 1  # GA_EINVAL, on the host before any launch
    assert L.ga_last_error().decode()


def test_more_than_32_replicas_is_unsupported():
    L = _lib.lib()
    assert _gram(L, K=33, ld=8, n=8) == 3  # GA_EUNSUP
    assert "33" in L.ga_last_error().decode()
    assert L.ga_replica_gram_workspace_bytes(33, 8) == -1


def test_zero_length_returns_ok():
    L = _lib.lib()
    assert L.ga_replica_gram(0, None, 2, 0, 0, None, None, None, None, None) == 0
    assert L.ga_last_error().decode() == ""
    assert L.ga_replica_gram_workspace_bytes(2, 0) == 0


def test_chain_bound_and_workspace():
    L = _lib.lib()
    chain = L.ga_replica_gram_chain()
    assert 1 <= chain <= 4096
    # one fp32 partial of K*K + 2K values per workgroup, at least one workgroup
    for K in (1, 8, 32):
        one = L.ga_replica_gram_workspace_bytes(K, 1)
        assert one == 4 * (K * K + 2 * K)
        big = L.ga_replica_gram_workspace_bytes(K, 124_000_000)
        assert big % one == 0 and big > one


def test_op_refuses_cpu_tensors():
    from gym_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.replica_gram(torch.zeros(2, 64))


@pytest.mark.parametrize("K", [2, 5])
def test_correlation_from_gram_matches_corrcoef(K):
    from gym_amd.metrics import correlation_from_gram
    rng = np.random.default_rng(K)
    x = rng.standard_normal((K, 1000)) + rng.standard_normal((K, 1))
    x[1] += 0.5 * x[0]
    gram, rowsum, _ = fake_metrics_ops.reference(x)
    got = correlation_from_gram(gram, rowsum, 1000)
    np.testing.assert_allclose(got, np.corrcoef(x), rtol=0, atol=1e-12)
    # zero padding beyond the real elements changes nothing
    xp = np.concatenate([x, np.zeros((K, 24))], axis=1)
    gram_p, rowsum_p, _ = fake_metrics_ops.reference(xp)
    np.testing.assert_allclose(correlation_from_gram(gram_p, rowsum_p, 1000), np.corrcoef(x), rtol=0, atol=1e-12)


def test_zero_variance_row_is_nan_like_corrcoef():
    from gym_amd.metrics import correlation_from_gram
    x = np.random.default_rng(0).standard_normal((3, 100))
    x[1] = 2.0
    gram, rowsum, _ = fake_metrics_ops.reference(x)
    got = correlation_from_gram(gram, rowsum, 100)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.corrcoef(x)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[1]).all() and np.isnan(got[:, 1]).all()
    assert abs(got[0, 2] - want[0, 2]) < 1e-12


@pytest.mark.parametrize("K_local", [1, 2])
def test_node_drift_over_gloo(tmp_path, K_local):
    """World of 3, K_local rows each: rank 0's dict equals numpy's on the same
    per-rank seeded vectors in node order, the other ranks get None."""
    import torch.multiprocessing as mp
    from strategy_scenarios import free_port
    world, ld, n, n_true = 3, 1024, 1000, 990
    mp.spawn(fake_metrics_ops.drift_worker, args=(world, free_port(), K_local, ld, n, n_true, str(tmp_path)),
             nprocs=world, join=True)
    res = [json.load(open(tmp_path / f"r{r}.json")) for r in range(world)]
    assert res[1] is None and res[2] is None
    x = torch.cat([fake_metrics_ops.rank_rows(r, K_local, ld, n, n_true) for r in range(world)])
    x = x[:, :n_true].double().numpy()
    N = world * K_local
    got = res[0]
    assert set(got) == {"correlation", "avg_model_correlation", "norm", "dist_to_mean", "consensus_distance"}
    corr = np.corrcoef(x)
    np.testing.assert_allclose(np.array(got["correlation"]), corr, rtol=0, atol=1e-12)
    assert abs(got["avg_model_correlation"] - corr[np.triu_indices(N, k=1)].mean()) < 1e-12
    np.testing.assert_allclose(got["norm"], np.linalg.norm(x, axis=1), rtol=1e-12)
    d = np.linalg.norm(x - x.mean(axis=0), axis=1)
    np.testing.assert_allclose(got["dist_to_mean"], d, rtol=1e-12)
    np.testing.assert_allclose(got["consensus_distance"], (d * d).mean(), rtol=1e-12)


class _World:
    def __init__(self, world):
        self.world, self.rank, self.exchange = world, 0, world > 1


def test_construction_errors():
    from gym_amd import NodeDrift
    with pytest.raises(Exception, match="Correlation calculation cannot be used with < 2 nodes"):
        NodeDrift(_World(1), 1, 64, 64, 64, torch.device("cpu"), torch.float32)
    with pytest.raises(ValueError, match="32"):
        NodeDrift(_World(11), 3, 64, 64, 64, torch.device("cpu"), torch.float32)
    NodeDrift(_World(16), 2, 64, 64, 64, torch.device("cpu"), torch.float32)  # 32 nodes: the limit itself


def test_run_log_records_metrics():
    from gym_amd.strategy import OptimSpec, SimpleReduceStrategy
    from gym_amd.train_node import RunLog
    log = RunLog(SimpleReduceStrategy(optim_spec=OptimSpec(torch.optim.SGD, lr=0.1)), 4)
    assert log.summary()["metrics"] == []
    log.increment_step()
    log.log_metric("consensus_distance", 0.5)
    s = log.summary()
    assert s["metrics"] == [(1, "consensus_distance", 0.5)]
    assert {"train", "evals", "lrs"} <= set(s)
