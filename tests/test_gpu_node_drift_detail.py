"""ga_replica_gram_centered on the MI355X (Gram matrix of the centred values on the
f32 MFMA, m . d, sum d, sum m^2, sum m) and the detailed node-drift metric end to end.

Exactness: integer rows whose node mean is an integer make every fp32 operation of the
kernel exact (test_integer_data_is_exact_fp32), so it must equal integer arithmetic bit
for bit on every path: both MFMA shapes (K <= 16, K > 16), one and several workgroups
(16384 columns each), waves (4096), tiles (256), the n % 4 tail, NaN padding beyond n,
vector and element loads.
Accuracy: the first-order bounds of tests/drift_bounds.py with L read from the library.
Close nodes: 1 - correlation and the pairwise distances of nodes 1e-3 and 1e-4 apart,
where the plain Gram path has lost them.
"""
import functools

import numpy as np
import pytest
import torch

import drift_bounds
import tiny_models

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 16, 17, 31, 32]
NS = [1, 3, 4, 65, 257, 4097, 16387, 200003]
CLASSIC = {"correlation", "avg_model_correlation", "norm", "dist_to_mean", "consensus_distance"}
DETAIL = CLASSIC | {"one_minus_correlation", "avg_model_decorrelation", "pairwise_distance",
                    "max_pairwise_distance"}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lds(n):
    return [n, (n + 63) // 64 * 64 + 64]


@functools.lru_cache(maxsize=None)
def _int_parts():
    """a [200003] integers in [-8, 8] and q [31, 200003] integers in [-1, 1] (int64, host)."""
    rng = np.random.default_rng(11)
    return rng.integers(-8, 9, size=max(NS), dtype=np.int64), rng.integers(-1, 2, size=(31, max(NS)), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _int_rows(K):
    """(x [K, 200003], d [K, 200003]) int64: x_k = a + q_k, the last q minus the sum of the
    others, so that sum_k x_k = K a and d_k = x_k - a = q_k."""
    a, q = _int_parts()
    d = np.concatenate([q[:K - 1], -q[:K - 1].sum(axis=0, keepdims=True)], axis=0)
    return a + d, d


@functools.lru_cache(maxsize=None)
def _int_reference(K, n):
    a = _int_parts()[0][:n]
    d = _int_rows(K)[1][:, :n]
    return d @ d.T, d @ a, d.sum(axis=1), np.array([a @ a, a.sum()])


def _place(x, ld, dtype, offset=0):
    """x [K, n] (host) as the first n columns of a [K, ld] device set whose other
    columns are NaN; offset moves the base pointer by that many elements."""
    K, n = x.shape
    buf = torch.full((K * ld + offset,), float("nan"), dtype=dtype, device="cuda")
    src = buf[offset:].view(K, ld)
    src[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).to(device="cuda", dtype=dtype)
    return src


def _run(src, n):
    from gym_amd import ops
    out = ops.replica_gram_centered(src, n=n)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _assert_exact(got, K, n, what):
    want = _int_reference(K, n)
    for name, g, w in zip(("cgram", "mdot", "dsum", "mstat"), got, want):
        assert g.dtype == np.float64 and g.shape == w.shape, (name, what)
        assert np.array_equal(g, w.astype(np.float64)), (name, what)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_integer_data_is_exact_fp32(K, n):
    """x_k = a + q_k with |a| <= 8, q_k in [-1, 1] for k < K - 1 and q_{K-1} = -sum of the
    others (|q_{K-1}| <= K - 1 <= 31).  The ascending fp32 sum of the x_k passes only
    through integers of magnitude <= 32 * 39 and ends at K a, and K a / K = a exactly
    under a correctly rounded division, so m = a and d_k = q_k for every K.  Every
    summand is then an integer, |d_i d_j| <= 961, |m d_k| <= 248, m^2 <= 64, and every
    fp32 partial covers at most 16384 columns: its running sums stay below
    961 * 16384 = 15 745 024 < 2^24 = 16 777 216 in magnitude, where fp32 holds every
    integer.  The fp64 final sum is far from 2^53.  So all four outputs must equal
    int64 arithmetic bit for bit."""
    _need_gpu()
    x = _int_rows(K)[0][:, :n]
    for ld in _lds(n):
        got = _run(_place(x, ld, torch.float32), n)
        _assert_exact(got, K, n, (K, n, ld))
        if K == 1:
            assert not got[0].any()


@pytest.mark.parametrize("n", [65, 4097, 200003])
@pytest.mark.parametrize("K", [4, 32])
def test_base_pointer_offset_by_one_element(K, n):
    """A base 4 bytes off 16-byte alignment takes the element-wise loads: same results."""
    _need_gpu()
    src = _place(_int_rows(K)[0][:, :n], _lds(n)[1], torch.float32, offset=1)
    assert src.data_ptr() % 16 == 4
    _assert_exact(_run(src, n), K, n, (K, n))


@pytest.mark.parametrize("n", [65, 4099])
@pytest.mark.parametrize("K", [3, 32])
def test_bf16_integer_data_is_exact(K, n):
    """|x| <= 39: bf16 holds these integers."""
    _need_gpu()
    x = _int_rows(K)[0][:, :n]
    for ld, offset in [(n, 0), (_lds(n)[1], 0), (_lds(n)[1], 1)]:
        _assert_exact(_run(_place(x, ld, torch.bfloat16, offset=offset), n), K, n, (K, n, ld, offset))


def test_zero_length_zeroes_the_outputs_and_too_many_rows_raise():
    _need_gpu()
    from gym_amd import ops
    got = _run(torch.full((3, 64), float("nan"), device="cuda"), 0)
    assert [g.shape for g in got] == [(3, 3), (3,), (3,), (2,)]
    assert not any(g.any() for g in got)
    with pytest.raises(ValueError, match="32"):
        ops.replica_gram_centered(torch.zeros(33, 64, device="cuda"))


@functools.lru_cache(maxsize=None)
def _randn(K):
    g = torch.Generator().manual_seed(100 + K)
    return torch.randn(K, 200003, generator=g).numpy()


@pytest.mark.parametrize("K", [8, 32])
def test_two_runs_give_identical_bits(K):
    _need_gpu()
    from gym_amd import ops
    src = _place(_randn(K), 200064, torch.float32)
    a = ops.replica_gram_centered(src, n=200003)
    b = ops.replica_gram_centered(src, n=200003)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("K", [8, 32])
def test_accuracy_against_float64(K):
    """Each output within the first-order bound of tests/drift_bounds.py, which the CPU
    suite has checked against a float32 emulation of the kernel's order."""
    _need_gpu()
    from gym_amd import ops
    L = ops.replica_gram_chain()
    assert 1 <= L <= 4096
    x = _randn(K)
    n = x.shape[1]
    got = _run(_place(x, n, torch.float32), n)
    ref, bound = drift_bounds.reference_and_bounds(x, L)
    for name, g, r, bd in zip(("cgram", "mdot", "dsum", "mstat"), got, ref, bound):
        err = np.abs(g - r)
        print(f"K={K} {name}: max err/bound {np.max(err / bd):.3g}")
        assert np.all(err <= bd), name
    assert np.array_equal(got[0], got[0].T)


def test_the_two_kernels_agree():
    """A + b_i + b_j + C_ij is ga_replica_gram's gram, S + t_k its rowsum, diag(C) its
    dist2, each within the sum of the two kernels' bounds."""
    _need_gpu()
    from gym_amd import ops
    K, n = 8, 200003
    x = _randn(K)
    src = _place(x, n, torch.float32)
    C, b, t, (A, S) = _run(src, n)
    gram, rowsum, dist2 = (o.cpu().numpy() for o in ops.replica_gram(src, n=n, want_dist=True))
    L = ops.replica_gram_chain()
    _, (bC, bb, bt, (bA, bS)) = drift_bounds.reference_and_bounds(x, L)
    _, (bG, bs, bd2) = drift_bounds.plain_reference_and_bounds(x, L)
    cases = (("gram", A + b[:, None] + b[None, :] + C, gram, bA + bb[:, None] + bb[None, :] + bC + bG),
             ("rowsum", S + t, rowsum, bS + bt + bs),
             ("dist2", np.diag(C), dist2, np.diag(bC) + bd2))
    for name, mine, theirs, bd in cases:
        err = np.abs(mine - theirs)
        print(f"{name}: max difference/bound {np.max(err / bd):.3g}")
        assert np.all(err <= bd), name


class _OneProcess:
    world, rank, exchange = 1, 0, False


@pytest.mark.parametrize("delta", [1e-3, 1e-4])
def test_close_nodes_keep_their_pairs(delta):
    """x_k = base + delta randn: 1 - corr_ij ~ delta^2 and |x_i - x_j| ~ delta |x|.  The
    centred kernel holds both to the 1e-3 the project holds dist_to_mean to (a float32
    emulation sits near 3e-6); from the plain Gram matrix and row sums they are noise,
    which is printed beside them, not asserted."""
    _need_gpu()
    from gym_amd import ops
    from gym_amd.metrics import NodeDrift, correlation_from_gram
    K, n = 8, 200003
    g = torch.Generator().manual_seed(5)
    base = torch.randn(1, n, generator=g)
    x = (base + delta * torch.randn(K, n, generator=g)).numpy()
    src = _place(x, n, torch.float32)
    out = NodeDrift(_OneProcess(), K, n, n, n, src.device, src.dtype, detail=True)(src)
    assert set(out) == DETAIL
    x64 = x.astype(np.float64)
    off = ~np.eye(K, dtype=bool)
    want_omc, want_pair = drift_bounds.one_minus_corr(x64)[off], drift_bounds.pairwise_distance(x64)[off]
    rel_omc = np.abs(np.array(out["one_minus_correlation"])[off] - want_omc) / want_omc
    rel_pair = np.abs(np.array(out["pairwise_distance"])[off] - want_pair) / want_pair
    gram, rowsum, _ = (o.cpu().numpy() for o in ops.replica_gram(src, n=n))
    dg = np.diag(gram)
    old_omc = np.abs((1.0 - correlation_from_gram(gram, rowsum, n))[off] - want_omc) / want_omc
    old_pair = np.abs(np.sqrt(np.maximum(0.0, dg[:, None] + dg[None, :] - 2.0 * gram))[off] - want_pair) / want_pair
    print(f"delta={delta}: 1 - corr ~ {want_omc.mean():.3g}; max relative error of 1 - corr {rel_omc.max():.3g} "
          f"(plain Gram path {old_omc.max():.3g}), of pairwise_distance {rel_pair.max():.3g} "
          f"(plain Gram path {old_pair.max():.3g})")
    assert np.all(rel_omc <= 1e-3)
    assert np.all(rel_pair <= 1e-3)
    assert abs(out["avg_model_decorrelation"] - want_omc.mean()) <= 1e-3 * want_omc.mean()
    assert abs(out["max_pairwise_distance"] - want_pair.max()) <= 1e-3 * want_pair.max()


def _metrics(run_log):
    return {(step, name): value for step, name, value in run_log["metrics"]}


def _replica_run(tmp_path, drift_detail):
    """Four nodes in this process, FedAvg islands of two averaged after every step; returns
    (every _node_drift result, the run log)."""
    import torch.distributed as dist

    from gym_amd.replica import ReplicaTrainNode
    from gym_amd.strategy import FedAvgStrategy, OptimSpec
    torch.manual_seed(0)
    ds = tiny_models.dataset()
    strategy = FedAvgStrategy(inner_optim=OptimSpec(torch.optim.SGD, lr=0.1), island_size=2, H=1)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg{int(drift_detail)}", rank=0, world_size=1)
    try:
        kw = dict(drift_detail=True) if drift_detail else {}
        node = ReplicaTrainNode(tiny_models.TinyMLP(), ds, ds, strategy, torch.device("cuda:0"), 0, 4, 4,
                                num_epochs=1, max_steps=5, batch_size=32, minibatch_size=16, val_size=32,
                                val_interval=100, correlation_interval=1, **kw)
        results, measure = [], node._node_drift
        node._node_drift = lambda: results.append(measure())
        node.train()
    finally:
        dist.destroy_process_group()
    return results, node.logger.summary()


def test_replica_mode_islands_show_as_exact_zeros(tmp_path):
    """After every step that ends in an island average each node equals its island
    partner bit for bit and no other node: the zeros of pairwise_distance off the
    diagonal form a perfect matching.  The first step averages nothing (the reference's
    `local_step % H == 0 and local_step > 0`, federated_averaging.py): there the four
    nodes, one SGD step from a common start on their own batches, are all apart."""
    _need_gpu()
    results, log = _replica_run(tmp_path, True)
    assert len(results) == 5
    for step, out in enumerate(results, start=1):
        assert set(out) == DETAIL
        pair = np.array(out["pairwise_distance"])
        assert np.array_equal(pair, pair.T) and not np.diag(pair).any()
        zero = (pair == 0.0) & ~np.eye(4, dtype=bool)
        assert np.array_equal(zero.sum(axis=1), np.full(4, 0 if step == 1 else 1)), (step, pair)
        assert np.all(pair[~zero & ~np.eye(4, dtype=bool)] > 0.0)
        omc = np.array(out["one_minus_correlation"])
        assert np.all(omc[zero] <= 1e-12) and np.all(omc[~zero & ~np.eye(4, dtype=bool)] > 0.0)
        assert out["max_pairwise_distance"] == pair.max() > 0.0
    names = ("avg_model_correlation", "consensus_distance", "avg_model_decorrelation", "max_pairwise_distance")
    got = _metrics(log)
    assert set(got) == {(s, name) for s in range(1, 6) for name in names}
    for s, out in enumerate(results, start=1):
        assert got[(s, "avg_model_decorrelation")] == out["avg_model_decorrelation"] > 0.0
        assert got[(s, "max_pairwise_distance")] == out["max_pairwise_distance"]


def test_replica_mode_without_the_flag_is_todays(tmp_path, monkeypatch):
    _need_gpu()
    from gym_amd import ops

    def boom(*a, **kw):
        raise AssertionError("replica_gram_centered launched without drift_detail")

    monkeypatch.setattr(ops, "replica_gram_centered", boom)
    results, log = _replica_run(tmp_path, False)
    assert all(set(out) == CLASSIC for out in results) and len(results) == 5
    assert set(_metrics(log)) == {(s, name) for s in range(1, 6)
                                  for name in ("avg_model_correlation", "consensus_distance")}


def test_fit_replica_mode_records_the_detail():
    """Trainer.fit carries drift_detail to the replica node of its worker process."""
    _need_gpu()
    from gym_amd import LocalTrainer
    from gym_amd.strategy import FedAvgStrategy, OptimSpec
    torch.manual_seed(0)
    ds = tiny_models.dataset()
    tr = LocalTrainer(tiny_models.TinyMLP(), ds, ds, start_port=21320)
    tr.fit(num_epochs=1, strategy=FedAvgStrategy(inner_optim=OptimSpec(torch.optim.SGD, lr=0.1), island_size=2, H=1),
           num_nodes=4, max_steps=4, device="cuda:0", devices=[0], batch_size=32, minibatch_size=16, val_size=32,
           val_interval=100, replicas_per_process=4, correlation_interval=2, drift_detail=True)
    got = _metrics(tr.run_log)
    names = ("avg_model_correlation", "consensus_distance", "avg_model_decorrelation", "max_pairwise_distance")
    assert set(got) == {(s, name) for s in (2, 4) for name in names}
    for s in (2, 4):
        assert 0.0 < got[(s, "avg_model_decorrelation")] <= 2.0
        assert got[(s, "max_pairwise_distance")] > 0.0
        assert abs(got[(s, "avg_model_correlation")] + got[(s, "avg_model_decorrelation")] - 1.0) <= 1e-12


def test_fit_process_mode_records_the_detail():
    """Two processes on cuda:0 with SimpleReduce stay identical: decorrelation and the
    pairwise distance are 0 at steps 3 and 6, on rank 0's log."""
    _need_gpu()
    from gym_amd import LocalTrainer
    from gym_amd.strategy import OptimSpec, SimpleReduceStrategy
    torch.manual_seed(0)
    ds = tiny_models.dataset()
    tr = LocalTrainer(tiny_models.TinyMLP(), ds, ds, start_port=21330)
    tr.fit(num_epochs=1, strategy=SimpleReduceStrategy(optim_spec=OptimSpec(torch.optim.SGD, lr=0.1)), num_nodes=2,
           max_steps=6, device="cuda:0", devices=[0], batch_size=32, minibatch_size=16, val_size=32, val_interval=100,
           replicas_per_process=1, correlation_interval=3, drift_detail=True)
    got = _metrics(tr.run_log)
    names = ("avg_model_correlation", "consensus_distance", "avg_model_decorrelation", "max_pairwise_distance")
    assert set(got) == {(s, name) for s in (3, 6) for name in names}
    for s in (3, 6):
        assert 0.0 <= got[(s, "avg_model_decorrelation")] <= 1e-12
        assert got[(s, "max_pairwise_distance")] == 0.0
        assert got[(s, "consensus_distance")] == 0.0
