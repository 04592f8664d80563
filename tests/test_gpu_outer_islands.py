"""Island DiLoCo on the MI355X: the replica runner's rounds (partners equal, islands
different, the pair and the loner), island_size=None against DiLoCoStrategy through
LocalTrainer.fit, and four nodes as 4 replicas in one process against 2 processes x 2
replicas over gloo on the one GPU.  The kernel itself: test_gpu_outer_islands_kernel.py."""
import copy
import os
import random

import numpy as np
import pytest
import torch

import island_checks as I

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 321


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gym_amd import _lib
    _lib.lib()


def _host(x):
    torch.cuda.synchronize()
    return x.detach().cpu().float().numpy()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32),
                          np.ascontiguousarray(b, np.float32).view(np.int32))


def _strategy(**kw):
    from gym_amd.strategy import IslandDiLoCoStrategy, OptimSpec
    return IslandDiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), **kw)


def _runner_rounds(K, steps, **kw):
    """ReplicaRunner over K nodes of the replica_scenarios model; the rows after every step
    and the launches of every round."""
    import replica_scenarios as R
    from gym_amd.engine import DiLoCoOuterIslands
    from gym_amd.replica import ReplicaRunner
    dev = torch.device(DEV)
    torch.manual_seed(42)
    random.seed(SEED)
    models = [R._model("x", dev) for _ in range(K)]
    runner = ReplicaRunner(_strategy(**kw), models, rank=0, num_nodes=K)
    assert type(runner.outer) is DiLoCoOuterIslands and runner.outer.master.shape == (K, runner.ra.ld)
    rows, launches = [], []
    for t in range(steps):
        runner.zero_grad()
        for k, m in enumerate(models):
            R._set_grads(m, k, t, dev)
        runner.outer.launch_elems = []
        runner.step()
        rows.append(_host(runner.ra.flat_set).copy())
        launches.append(list(runner.outer.launch_elems))
    return rows, launches, runner


def test_replica_runner_four_nodes_islands_of_two():
    rows, launches, runner = _runner_rounds(4, 6, island_size=2, H=2)
    random.seed(SEED)
    draws = [I.draw(4, 2) for _ in range(2)]
    ld = runner.ra.ld
    assert launches == [[], [], [ld], [], [ld], []]  # ONE launch per round, none between
    a, b = draws[0]
    first = rows[2]
    assert _same(first[a[0]], first[a[1]]) and _same(first[b[0]], first[b[1]])  # partners bit-equal
    assert not _same(first[a[0]], first[b[0]])                                  # the islands differ
    assert all(np.isfinite(r).all() for r in rows)
    # every node continues from its own master
    assert _same(rows[4], _host(runner.outer.master)) and not runner.outer.first
    p, q = draws[1][0]
    assert not _same(rows[4][p], rows[4][q])  # later partners differ: their masters do


def test_replica_runner_three_nodes_the_pair_and_the_loner():
    rows, launches, runner = _runner_rounds(3, 3, island_size=2, H=2)
    random.seed(SEED)
    pair, loner = I.draw(3, 2)
    assert len(pair) == 2 and len(loner) == 1 and launches == [[], [], [runner.ra.ld]]
    after = rows[2]
    assert _same(after[pair[0]], after[pair[1]]) and not _same(after[loner[0]], after[pair[0]])
    assert not _same(after[loner[0]], rows[1][loner[0]]) and np.isfinite(after).all()


def _fit(strategy, port):
    from tiny_models import TinyMLP, dataset
    from gym_amd.trainer import LocalTrainer
    torch.manual_seed(0)
    tr = LocalTrainer(TinyMLP(), dataset(256), dataset(64, seed=1), start_port=port)
    final = tr.fit(num_epochs=1, strategy=strategy, num_nodes=2, max_steps=10, devices=[0], batch_size=16,
                   minibatch_size=16, val_size=16, val_interval=100, replicas_per_process=2, keep_node_states=True)
    return tr.node_states, final


def test_one_island_through_fit_is_diloco():
    """island_size=None, both nodes in one process, TinyMLP, H = 4, 10 steps: every node's
    master stays the same, so the run is DiLoCoStrategy's bit for bit."""
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    got, final = _fit(_strategy(island_size=None, H=4), 22800)
    want, final_ref = _fit(DiLoCoStrategy(optim_spec=OptimSpec(torch.optim.AdamW, lr=1e-2), H=4), 22820)
    assert len(got) == len(want) == 2
    for r in range(2):
        for name in got[r]:
            assert torch.equal(got[r][name], want[r][name]), (r, name)
    for a, b in zip(final.parameters(), final_ref.parameters()):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    assert any(not torch.equal(got[0][k], got[1][k]) for k in got[0])  # two inner steps after the last round


FIT_KW = dict(num_epochs=1, max_steps=7, batch_size=16, minibatch_size=16, val_size=16, val_interval=100)


def _train_replicas(rank, procs):
    """What Trainer.fit's replica worker runs, for the K = 4 / procs nodes of process `rank`."""
    from tiny_models import TinyMLP, dataset
    from gym_amd.replica import ReplicaTrainNode
    torch.manual_seed(0)
    random.seed(SEED)  # the first process's draw
    node = ReplicaTrainNode(TinyMLP(), dataset(256), dataset(64, seed=1), _strategy(island_size=2, H=2),
                            torch.device(DEV), rank, 4, 4 // procs, **FIT_KW)
    states = node.train()
    torch.cuda.synchronize()
    return [{k: v.detach().cpu() for k, v in sd.items()} for sd in states], node.runner


def _two_by_two_worker(rank, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(torch.device(DEV))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        states, runner = _train_replicas(rank, 2)
        assert runner.coll.exchange and runner.outer.K_local == 2
        torch.save(states, os.path.join(out_dir, f"states{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_four_replicas_in_one_process_equal_two_processes_of_two(tmp_path):
    """4 nodes, islands of 2, H = 2, 7 steps (three rounds, one inner step after the last)
    of the trainer's replica node loop on TinyMLP: all four nodes in this process against
    2 processes x 2 replicas over gloo on the one GPU, started by this test (Trainer.fit
    places one process per GPU) with the same seed for the first process's draw.  An
    island's ascending-node sum has one order however the nodes are split, so every
    node's final state and the averaged final model are bit-identical."""
    import torch.multiprocessing as mp
    from gym_amd.trainer import _average_model_states
    mp.spawn(_two_by_two_worker, args=(22840, str(tmp_path)), nprocs=2, join=True)  # 2 processes on the GPU
    split = [sd for r in range(2) for sd in torch.load(tmp_path / f"states{r}.pt")]
    one, runner = _train_replicas(0, 1)
    assert len(one) == len(split) == 4 and not runner.coll.exchange
    for r in range(4):
        for name in one[r]:
            assert torch.equal(one[r][name], split[r][name]), (r, name)
            assert torch.isfinite(one[r][name]).all()
    a = _average_model_states(dict(enumerate(copy.deepcopy(one))))
    b = _average_model_states(dict(enumerate(split)))
    assert all(torch.equal(a[k], b[k]) for k in a)
    random.seed(SEED)
    last = [I.draw(4, 2) for _ in range(3)][-1]
    p, q = last[0]
    assert any(not torch.equal(one[p][k], one[last[1][0]][k]) for k in one[p])  # the islands went their own ways
