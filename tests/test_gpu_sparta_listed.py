"""The listed SPARTA step on the MI355X: both kernels bit for bit against sparta_checks'
numpy restatement, sentinel padding included; the cycle selectors in replica mode, listed
against the mask path; the exchange path at world size 1 against the local step."""
import os

import numpy as np
import pytest
import torch

import replica_scenarios as R
import sparta_checks as sc
from strategy_scenarios import free_port

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
SENT = 7.0
# 300 tensors at 64-aligned offsets; numels 1-3 among them, so one wave crosses many rows
NUMELS = [(1, 2, 3, 70, 129)[t % 5] for t in range(300)]
OFFS = [64 * 3 * t for t in range(300)]
N = OFFS[-1] + 129 + 11


def _tables():
    """order (a permutation of each tensor's arena indices at its offset) and the steps'
    {start, count} rows by name:
      dense  every tensor's slice [numel // 3, numel) (count >= 1): 300 rows, more than the
             256 a workgroup stages, total = 8280 = 129 * 64 + 24;
      gaps   the same with count 0 on rows 5 .. 289: a tile's rows run past its window;
      empty  total == 0."""
    rng = np.random.default_rng(3)
    order = np.full(N, -1, np.int32)
    for o, m in zip(OFFS, NUMELS):
        order[o:o + m] = o + rng.permutation(m)
    dense = [(o + m // 3, m - m // 3) for o, m in zip(OFFS, NUMELS)]
    gaps = [(s, 0 if 5 <= t < 290 else c) for t, (s, c) in enumerate(dense)]
    return order, {"dense": dense, "gaps": gaps, "empty": []}


def _table(rows):
    pre = np.concatenate([[0], np.cumsum([c for _, c in rows])[:-1]]) if rows else np.zeros(0)
    t = np.array([(s, c, p) for (s, c), p in zip(rows, pre)], np.int32).reshape(-1, 3)
    return torch.from_numpy(t).to(DEV), int(sum(c for _, c in rows))


def _set(x, dtype, layout):
    """(buffer, set view) of x [K, N]: rows [K, N + 61] or element-major [N + 3, K + 5]; SENT elsewhere."""
    K = x.shape[0]
    full = np.full((N + 3, K + 5) if layout == "elem" else (K, N + 61), SENT, np.float32)
    if layout == "elem":
        full[:N, :K] = x.T
    else:
        full[:, :N] = x
    buf = torch.from_numpy(full).to(DEV, dtype)
    return buf, (buf[:, :K] if layout == "elem" else buf)


def _same(buf, want, K, layout):
    got = buf.float().cpu().numpy()
    got, pad = (got[:N, :K].T, got.copy()) if layout == "elem" else (got[:, :N], got.copy())
    (pad[:N, :K] if layout == "elem" else pad[:, :N])[...] = SENT
    return np.array_equal(sc.bits_of(got), sc.bits_of(want)) and (pad == SENT).all()


@pytest.mark.parametrize("twice", [False, True], ids=["divK", "div2K"])
@pytest.mark.parametrize("K", [1, 3, 33])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("layout", ["rows", "elem"])
def test_listed_kernels_match_numpy(layout, dtype, K, twice):
    from gym_amd import ops
    dt, divisor = DTYPES[dtype], float(2 * K if twice else K)
    order_np, steps = _tables()
    order = torch.from_numpy(order_np).to(DEV)
    x = np.random.default_rng(K).standard_normal((K, N), dtype=np.float32)
    for name, rows in steps.items():
        table, total = _table(rows)
        listed = np.concatenate([order_np[s:s + c] for s, c in rows] + [np.zeros(0, np.int32)])
        m = np.zeros(N, bool)
        m[listed] = True
        assert m.sum() == total == len(listed) and total == {"dense": 8280, "gaps": 414, "empty": 0}[name]
        buf, view = _set(sc.round_to(x, dt), dt, layout)
        ops.sparta_average_listed(view, order, table, total, divisor, n=N, layout=layout)
        assert _same(buf, sc.expect_fused(x, m, divisor, dt), K, layout), (name, "average")
        # gather -> scatter: vals = RN_dtype(fp32 sum) in list order, then RN_dtype(vals / divisor)
        buf, view = _set(sc.round_to(x, dt), dt, layout)
        idx = torch.full((total + 8,), -7, dtype=torch.int32, device=DEV)
        vals = torch.full((total + 8,), -3.0, dtype=dt, device=DEV)
        count = torch.full((2,), -1, dtype=torch.int64, device=DEV)
        ops.sparta_gather_listed(view, order, table, total, idx, vals, count, n=N, layout=layout)
        want_vals, two = sc.expect_two_step(x, m, divisor, dt)
        assert _same(buf, sc.round_to(x, dt), K, layout), (name, "gather only reads")
        assert count.tolist() == ([total, 0] if total else [-1, -1]), name
        assert np.array_equal(idx.cpu().numpy(), np.concatenate([listed, np.full(8, -7)])), name
        by_elem = want_vals[np.searchsorted(np.flatnonzero(m), listed)] if total else want_vals
        assert np.array_equal(sc.bits_of(vals.float().cpu().numpy()),
                              sc.bits_of(np.concatenate([by_elem, np.full(8, -3.0, np.float32)]))), name
        if total:
            ops.sparta_scatter(vals, idx, count, total, divisor, view, layout=layout)
        assert _same(buf, two, K, layout), (name, "scatter")


def _run_replicas(cls, p, listed, steps, K=4):
    from gym_amd.replica import ReplicaRunner
    from gym_amd.strategy import OptimSpec, SPARTAStrategy
    torch.manual_seed(42)
    dev = torch.device(DEV)
    models = [R._model("x", dev) for _ in range(K)]
    s = SPARTAStrategy(inner_optim=OptimSpec(torch.optim.AdamW, lr=1e-2), p_sparta=p)
    s.index_selector = s.communication_modules[0].index_selector = cls(p, listed=listed)
    runner = ReplicaRunner(s, models, rank=0, num_nodes=K)
    for t in range(steps):
        runner.zero_grad()
        for k, m in enumerate(models):
            R._set_grads(m, k, t, dev)
        runner.step()
    return ([[q.detach().cpu().numpy() for q in m.parameters()] for m in models], runner.sparta.mask_draw,
            torch.cuda.get_rng_state(dev))


@pytest.mark.parametrize("name", ["ShuffledSequentialIndexSelector", "PartitionedIndexSelector"])
def test_replica_mode_listed_equals_mask_path(name):
    """p = 0.04: 25 partitions, more than the 21 elements of the (3, 7) tensor; 52 steps:
    a ShuffledSequential wrap and Partitioned redraws (every 25 steps, every 21 for (3, 7))."""
    from gym_amd.strategy import sparta
    cls, p = getattr(sparta, name), 0.04
    a, draw_a, gen_a = _run_replicas(cls, p, True, 2 * 25 + 2)
    b, draw_b, gen_b = _run_replicas(cls, p, False, 2 * 25 + 2)
    assert draw_a == "listed" and draw_b == "torch"
    assert torch.equal(gen_a, gen_b)
    for node_a, node_b in zip(a, b):
        for x, y in zip(node_a, node_b):
            assert np.array_equal(sc.bits_of(x), sc.bits_of(y))


def _exchange_worker(rank, port):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    from gym_amd.arena import ArenaLayout
    from gym_amd.comm import Collective
    from gym_amd.strategy.sparta import PartitionedIndexSelector, SparseAverage
    dev = torch.device(DEV)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        L = ArenaLayout(R.SHAPES)
        params = [torch.zeros(s, device=dev, requires_grad=True) for s in R.SHAPES]
        for q in params:
            q.grad = torch.zeros_like(q)
        out = []
        for force in (False, True):
            torch.manual_seed(7)
            reps = torch.randn(3, L.n, generator=torch.Generator().manual_seed(1)).to(dev)
            sp = SparseAverage()
            sp.bind(PartitionedIndexSelector(0.25, listed=True), Collective(force_exchange=force), 3, L, L.n, dev,
                    torch.float32)
            for _ in range(5):  # a redraw at the fifth step: rank 0's ranges broadcast again
                sp(reps, params)
                sp.iteration += 1
            assert sp.mask_draw == "listed" and sp.engine.coll.exchange is force
            out.append(reps)
        assert torch.equal(out[0], out[1])
        assert torch.equal(out[1][0], out[1][2]) is False and (out[1][0] == out[1][2]).sum() >= L.n_params
    finally:
        dist.destroy_process_group()


def test_exchange_path_world1_equals_local_step():
    import torch.multiprocessing as mp
    mp.spawn(_exchange_worker, args=(free_port(),), nprocs=1, join=True)
