"""ga_replica_gram on the MI355X (Gram matrix on the f32 MFMA, row sums, squared
distances to the node mean) and the node-drift metric end to end.

Exactness: integer data in [-2, 2] makes every fp32 sum exact, so the kernel must
equal integer arithmetic bit for bit on every path: both MFMA shapes (K <= 16,
K > 16), one and several workgroups (16384 columns each), tiles (256 columns),
the n % 4 tail, NaN padding beyond n, vector and element loads.
Accuracy: the fp32 fma-chain bound of include/gym_amd.h with L read from the library.
"""
import functools

import numpy as np
import pytest
import torch

import tiny_models

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 8, 16, 17, 32]
NS = [1, 3, 4, 63, 64, 65, 4099, 200003]
U = 2.0 ** -24


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lds(n):
    return [n, (n + 63) // 64 * 64 + 64]


@functools.lru_cache(maxsize=None)
def _ints():
    """[32, 200003] integers in [-2, 2] (int64, host); every case uses a corner of it."""
    return np.random.default_rng(7).integers(-2, 3, size=(32, max(NS)), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _int_reference(n):
    """int64 Gram and row sums of all 32 rows at length n: the K x K Gram of the
    first K rows is its top-left block."""
    x = _ints()[:, :n]
    return x @ x.T, x.sum(axis=1)


def _dist2_reference(K, n):
    x = _ints()[:K, :n].astype(np.float64)
    c = x - x.sum(axis=0) / K  # exact for K a power of two
    return (c * c).sum(axis=1)


def _place(x, ld, dtype, offset=0):
    """x [K, n] (host) as the first n columns of a [K, ld] device set whose other
    columns are NaN; offset moves the base pointer by that many elements."""
    K, n = x.shape
    buf = torch.full((K * ld + offset,), float("nan"), dtype=dtype, device="cuda")
    src = buf[offset:].view(K, ld)
    src[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).to(device="cuda", dtype=dtype)
    return src


def _run(src, n, want_dist=True):
    from gym_amd import ops
    gram, rowsum, dist2 = ops.replica_gram(src, n=n, want_dist=want_dist)
    torch.cuda.synchronize()
    return gram.cpu().numpy(), rowsum.cpu().numpy(), (dist2.cpu().numpy() if dist2 is not None else None)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_integer_data_is_exact_fp32(K, n):
    _need_gpu()
    G, s = _int_reference(n)
    x = _ints()[:K, :n]
    for ld in _lds(n):
        gram, rowsum, dist2 = _run(_place(x, ld, torch.float32), n)
        assert gram.dtype == np.float64 and gram.shape == (K, K)
        assert np.array_equal(gram, G[:K, :K].astype(np.float64)), (K, n, ld)
        assert np.array_equal(rowsum, s[:K].astype(np.float64)), (K, n, ld)
        if K in (2, 4, 8):
            assert np.array_equal(dist2, _dist2_reference(K, n)), (K, n, ld)
        elif K == 1:
            assert np.array_equal(dist2, np.zeros(1))


@pytest.mark.parametrize("n", [65, 4099, 200003])
@pytest.mark.parametrize("K", [4, 32])
def test_base_pointer_offset_by_one_element(K, n):
    """A base 4 bytes off 16-byte alignment takes the element-wise loads: same results."""
    _need_gpu()
    G, s = _int_reference(n)
    ld = _lds(n)[1]
    src = _place(_ints()[:K, :n], ld, torch.float32, offset=1)
    assert src.data_ptr() % 16 == 4
    gram, rowsum, dist2 = _run(src, n)
    assert np.array_equal(gram, G[:K, :K].astype(np.float64))
    assert np.array_equal(rowsum, s[:K].astype(np.float64))
    if K == 4:
        assert np.array_equal(dist2, _dist2_reference(K, n))


@pytest.mark.parametrize("n", [65, 4099])
@pytest.mark.parametrize("K", [3, 32])
def test_bf16_integer_data_is_exact(K, n):
    _need_gpu()
    G, s = _int_reference(n)
    x = _ints()[:K, :n]
    for ld, offset in [(n, 0), (_lds(n)[1], 0), (_lds(n)[1], 1)]:
        gram, rowsum, _ = _run(_place(x, ld, torch.bfloat16, offset=offset), n)
        assert np.array_equal(gram, G[:K, :K].astype(np.float64)), (K, n, ld, offset)
        assert np.array_equal(rowsum, s[:K].astype(np.float64)), (K, n, ld, offset)


def test_dist2_exact_at_k4_and_skipped_when_not_wanted():
    _need_gpu()
    n = 4099
    src = _place(_ints()[:4, :n], n, torch.float32)
    gram, rowsum, dist2 = _run(src, n)
    assert np.array_equal(dist2, _dist2_reference(4, n))
    gram2, rowsum2, none = _run(src, n, want_dist=False)
    assert none is None and np.array_equal(gram, gram2) and np.array_equal(rowsum, rowsum2)


def test_zero_length_zeroes_the_outputs_and_too_many_rows_raise():
    _need_gpu()
    from gym_amd import ops
    gram, rowsum, dist2 = _run(torch.full((3, 64), float("nan"), device="cuda"), 0)
    assert not gram.any() and not rowsum.any() and not dist2.any()
    with pytest.raises(ValueError, match="32"):
        ops.replica_gram(torch.zeros(33, 64, device="cuda"))


@functools.lru_cache(maxsize=None)
def _randn(K):
    g = torch.Generator().manual_seed(100 + K)
    return torch.randn(K, 200003, generator=g).numpy()


@pytest.mark.parametrize("K", [8, 32])
def test_two_runs_give_identical_bits(K):
    _need_gpu()
    from gym_amd import ops
    src = _place(_randn(K), 200064, torch.float32)
    a = ops.replica_gram(src, n=200003)
    b = ops.replica_gram(src, n=200003)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("K", [8, 32])
def test_accuracy_against_float64(K):
    """|G - G64| <= (L + 16) 2^-24 sum |x_i x_j|: the first-order bound of an fma
    chain of L products plus the in-workgroup combines; dist2 likewise on the centred
    values, plus the rounding of the centring itself."""
    _need_gpu()
    from gym_amd import ops
    L = ops.replica_gram_chain()
    assert 1 <= L <= 4096
    x = _randn(K)
    n = x.shape[1]
    gram, rowsum, dist2 = _run(_place(x, n, torch.float32), n)
    x64 = x.astype(np.float64)
    G64 = x64 @ x64.T
    bound = (L + 16) * U * (np.abs(x64) @ np.abs(x64).T)
    err = np.abs(gram - G64)
    print(f"K={K} gram: max err/bound {np.max(err / bound):.3g}")
    assert np.all(err <= bound)
    assert np.array_equal(gram, gram.T)
    np.testing.assert_allclose(rowsum, x64.sum(axis=1), rtol=0, atol=(L + 16) * U * np.abs(x64).sum(axis=1).max())
    m = x64.sum(axis=0) / K
    c = x64 - m
    d64 = (c * c).sum(axis=1)
    dbound = (L + 16) * U * d64 + 8 * U * (np.abs(c) * (np.abs(x64) + np.abs(m))).sum(axis=1)
    derr = np.abs(dist2 - d64)
    print(f"K={K} dist2: max err/bound {np.max(derr / dbound):.3g}")
    assert np.all(derr <= dbound)


def test_close_nodes_keep_their_distance():
    """x_k = base + 1e-3 randn: the distance to the mean is ~1e-3 of the norm, where
    G_kk - 2 x_k.m + m.m from an fp32-chain Gram cancels; the centred sum does not."""
    _need_gpu()
    K, n = 8, 200003
    g = torch.Generator().manual_seed(5)
    base = torch.randn(1, n, generator=g)
    x = (base + 1e-3 * torch.randn(K, n, generator=g)).numpy()
    _, _, dist2 = _run(_place(x, n, torch.float32), n)
    x64 = x.astype(np.float64)
    d64 = np.sqrt(((x64 - x64.mean(axis=0)) ** 2).sum(axis=1))
    rel = np.abs(np.sqrt(dist2) - d64) / d64
    print(f"close nodes: max relative error of dist_to_mean {rel.max():.3g}")
    assert np.all(rel <= 1e-3)


def _metrics(run_log):
    return {(step, name): value for step, name, value in run_log["metrics"]}


def test_fit_process_mode_records_drift():
    """Two processes on cuda:0 with SimpleReduce stay identical: correlation 1,
    consensus distance exactly 0, recorded at steps 3 and 6."""
    _need_gpu()
    from gym_amd import LocalTrainer
    from gym_amd.strategy import OptimSpec, SimpleReduceStrategy
    torch.manual_seed(0)
    ds = tiny_models.dataset()
    tr = LocalTrainer(tiny_models.TinyMLP(), ds, ds, start_port=21300)
    tr.fit(num_epochs=1, strategy=SimpleReduceStrategy(optim_spec=OptimSpec(torch.optim.SGD, lr=0.1)), num_nodes=2,
           max_steps=6, device="cuda:0", devices=[0], batch_size=32, minibatch_size=16, val_size=32, val_interval=100,
           replicas_per_process=1, correlation_interval=3)
    got = _metrics(tr.run_log)
    assert set(got) == {(s, name) for s in (3, 6) for name in ("avg_model_correlation", "consensus_distance")}
    for s in (3, 6):
        assert abs(got[(s, "avg_model_correlation")] - 1.0) <= 1e-6
        assert got[(s, "consensus_distance")] == 0.0


def test_fit_replica_mode_records_drift():
    """Four nodes in one process, FedAvg(H=4): apart at step 3 (before the first average)."""
    _need_gpu()
    from gym_amd import LocalTrainer
    from gym_amd.strategy import FedAvgStrategy, OptimSpec
    torch.manual_seed(0)
    ds = tiny_models.dataset()
    tr = LocalTrainer(tiny_models.TinyMLP(), ds, ds, start_port=21310)
    tr.fit(num_epochs=1, strategy=FedAvgStrategy(inner_optim=OptimSpec(torch.optim.SGD, lr=0.1), H=4), num_nodes=4,
           max_steps=6, device="cuda:0", devices=[0], batch_size=32, minibatch_size=16, val_size=32, val_interval=100,
           replicas_per_process=4, correlation_interval=3)
    got = _metrics(tr.run_log)
    assert set(got) == {(s, name) for s in (3, 6) for name in ("avg_model_correlation", "consensus_distance")}
    for s in (3, 6):
        assert -1.0 <= got[(s, "avg_model_correlation")] <= 1.0
    assert got[(3, "consensus_distance")] > 0.0


def test_interval_unset_builds_nothing(monkeypatch, tmp_path):
    """Without correlation_interval no NodeDrift is constructed and nothing is recorded."""
    _need_gpu()
    import torch.distributed as dist

    import gym_amd.metrics as metrics
    from gym_amd.replica import ReplicaTrainNode
    from gym_amd.strategy import FedAvgStrategy, OptimSpec

    def boom(self, *a, **kw):
        raise AssertionError("NodeDrift constructed without correlation_interval")

    monkeypatch.setattr(metrics.NodeDrift, "__init__", boom)
    torch.manual_seed(0)
    ds = tiny_models.dataset()
    strategy = FedAvgStrategy(inner_optim=OptimSpec(torch.optim.SGD, lr=0.1), H=2)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        node = ReplicaTrainNode(tiny_models.TinyMLP(), ds, ds, strategy, torch.device("cuda:0"), 0, 2, 2,
                                num_epochs=1, max_steps=4, batch_size=32, minibatch_size=16, val_size=32,
                                val_interval=100)
        node.train()
    finally:
        dist.destroy_process_group()
    assert node.drift is None
    assert node.logger.summary()["metrics"] == []
    assert len(node.logger.summary()["train"]) == 4
