"""outer_compression="lowrank" through Trainer.fit on the MI355X (the MNIST CNN, H = 2, rank 4
with error feedback), and one process per node against K nodes in one process."""
import numpy as np
import pytest
import torch

import lowrank_checks as C

pytestmark = pytest.mark.gpu
STEPS, H = 5, 2
SHAPES = [(33, 70), (64, 256), (40, 3, 3, 3), (5,), (1, 300)]
HP = dict(lr=0.7, momentum=0.9, nesterov=True, dampening=0.0, weight_decay=1e-3)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _fit(cls, nodes, replicas, port, **kw):
    """(every node's final parameters, the strategy)."""
    from tiny_models import MnistCNN, mnist_like
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    from gym_amd.trainer import LocalTrainer
    inner = OptimSpec(torch.optim.SGD, lr=1e-2)
    opts = dict(H=H, outer_compression="lowrank", outer_rank=4, outer_error_feedback=True, outer_lowrank_seed=7, **kw)
    s = cls(inner_optim=inner, **opts) if cls else DiLoCoStrategy(optim_spec=inner, **opts)
    torch.manual_seed(0)
    tr = LocalTrainer(MnistCNN(), mnist_like(192), mnist_like(32, seed=1), start_port=port)
    tr.fit(num_epochs=1, strategy=s, num_nodes=nodes, max_steps=STEPS, devices=[0], batch_size=8, minibatch_size=8,
           val_size=8, val_interval=100, replicas_per_process=replicas, keep_node_states=True)
    params = [n for n, _ in MnistCNN().named_parameters()]
    return [{n: sd[n] for n in params} for sd in tr.node_states], s


@pytest.mark.parametrize("nodes,replicas", [(4, 4), (2, 1)])
def test_fit_ends_on_an_outer_step_with_all_nodes_bit_equal(nodes, replicas):
    """K = 4 in one process, and 2 processes x 1 node over gloo.  The last step (local_step =
    STEPS - 1) is an outer step, so every node holds the new master's bits."""
    assert (STEPS - 1) % H == 0 and STEPS - 1 > 0
    got, s = _fit(None, nodes, replicas, 23100 + 20 * nodes)
    cfg = s.__config__()
    assert cfg["outer_rank"] == 4 and cfg["outer_lowrank_seed"] == 7 and cfg["outer_compression"] == "lowrank"
    assert len(got) == nodes and all(torch.isfinite(v).all() for v in got[0].values())
    assert all(torch.equal(got[0][n], got[k][n]) for k in range(1, nodes) for n in got[0])


def test_sparta_diloco_takes_a_boundary_step():
    from gym_amd.strategy import SPARTADiLoCoStrategy
    got, _ = _fit(SPARTADiLoCoStrategy, 2, 2, 23200, p_sparta=0.01)
    assert all(torch.isfinite(v).all() for sd in got for v in sd.values())
    assert all(torch.equal(got[0][n], got[1][n]) for n in got[0])


def _engine_steps(coll, K, rows, master, first_row=0):
    """Two engine steps on rows[step][first_row : first_row + K]; the state as numpy arrays."""
    from gym_amd.arena import ArenaLayout
    from gym_amd.engine import DiLoCoOuterLowRank
    L = ArenaLayout(SHAPES)
    eng = DiLoCoOuterLowRank(coll, K, L.n, "cuda", torch.float32, layout=L, rank=4, seed=1, error_feedback=True, **HP)
    eng.init_master(torch.from_numpy(master).cuda())
    for X in rows:
        eng(torch.from_numpy(X[first_row:first_row + K]).cuda())
    return {k: v.cpu().numpy() for k, v in dict(m=eng.master, b=eng.mom, E=eng.residual, B=eng.B).items()}


def _rank(rank, port, path, rows, master):
    import torch.distributed as dist
    from gym_amd.comm import Collective
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    np.savez(f"{path}.{rank}.npz", **_engine_steps(Collective(), 1, rows, master, rank))
    dist.destroy_process_group()


def test_two_processes_agree_with_two_replicas_at_the_engine(tmp_path):
    """The MNIST CNN's forward and backward are not bit-reproducible between the modes (plain
    DiLoCo differs too), so a fit cannot feed both the same rows; the engines are compared
    instead, on identical rows, over two steps (the second uses the residual and B / K_total).
    2 processes x 1 node over gloo sum the two products, K = 2 in one process multiplies the
    sum: each is held to 8x the deviation from float64 of the float32 restatement of its own
    order, the ranks to each other bit for bit."""
    from gym_amd.arena import ArenaLayout
    from gym_amd.comm import Collective
    from gym_amd.lowrank import LowRankPlan
    L, rng = ArenaLayout(SHAPES), np.random.default_rng(3)
    plan = LowRankPlan(L.shapes, L.offsets, L.n, 4)
    tensors = np.zeros(L.n, bool)
    for o, n in zip(L.offsets, L.numels):
        tensors[o:o + n] = True
    master = (rng.standard_normal(L.n) * tensors).astype(np.float32)
    rows = [(master + 1e-2 * rng.standard_normal((2, L.n)) * tensors).astype(np.float32) for _ in range(2)]
    torch.multiprocessing.spawn(_rank, args=(23260, str(tmp_path / "rank"), rows, master), nprocs=2, join=True)
    ranks = [dict(np.load(tmp_path / f"rank.{r}.npz")) for r in range(2)]
    assert all(np.array_equal(ranks[0][k], ranks[1][k]) for k in "mbB")
    procs = dict(ranks[0], E=np.concatenate([ranks[0]["E"], ranks[1]["E"]]))
    for got, split in ((_engine_steps(Collective(), 2, rows, master), False), (procs, True)):
        st = {d: dict(m=master.astype(d), b=None, E=np.zeros((2, L.n), d), B=plan.warm_start(1).numpy().astype(d))
              for d in (np.float64, np.float32)}
        for i, X in enumerate(rows):
            for d, s in st.items():
                s["E"], s["m"], s["b"], s["B"] = C.step(plan, s["m"], X, s["E"], s["B"], 2.0 if i else 1.0, s["b"], HP,
                                                        i == 0, d, split and d is np.float32)
        for k, ref in st[np.float64].items():
            own, err = np.abs(st[np.float32][k] - ref).max(), np.abs(got[k] - ref).max()
            print(f"{'2 processes' if split else 'K = 2'} {k}: deviation / float32 restatement's {err / own:.2f}")
            assert err <= 8 * own, (split, k)
