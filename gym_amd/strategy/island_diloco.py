"""Island DiLoCo: DiLoCo's local steps, and every H steps an outer step per node
against the average of a small random island instead of the world.

No reference counterpart (the reference's DiLoCo averages the world, diloco.py:34-37,
and its only island exchange, FedAvg's, has no outer optimizer).  The update is in the
gossip / NoLoCo family of low-communication methods, defined here, not a restatement
of any paper's equations:

IslandDiLoCoStrategy(optim_spec=None, outer_optim_spec=None, H=100, island_size=2,
**kwargs).  The inner loop is DiLoCoStrategy's (build_inner_optimizer, "max_norm"
clipping through clip_and_step).  Every node keeps an fp32 master and, with momentum,
an fp32 momentum buffer of its OWN, both started from node 0's initial parameters.
When local_step % H == 0 and local_step > 0, after the inner step, rank 0 draws the
islands exactly as FedAvg does (random.shuffle of the node ids, broadcast, consecutive
slices of island_size, the last may be short; island_size None or >= num_nodes: one
island of all nodes, no draw), the members of an island bring their arenas together
(FedAvg's cached island sub-communicators, or its world all-gather fallback), and every
node takes the SGD / Nesterov outer update of its own master against the island's
average -- the ascending-node fp32 sum over the island's size -- and continues from its
master.  One launch per node and round (ga_diloco_outer_islands); in
gym_amd.replica one launch per process and round for all its nodes.

Per round a node receives (s - 1) n elements instead of taking part in an all-reduce
over K nodes, no collective is world-wide once the sub-communicators exist, and a slow
node holds up its island only.  The price is 8 B of fp32 state per parameter and NODE.

Only plain torch.optim.SGD outer specs have a kernel (fused_sgd_hparams); anything
else, and the options of DiLoCoStrategy that have no island form (outer_compression,
outer_error_feedback, num_fragments, outer_delay, outer_mix), raise ValueError at
construction and again at node init.
"""
from typing import Optional, Union

from ..engine import DiLoCoOuterIslands
from .communicate_optimize_strategy import CommunicateOptimizeStrategy
from .diloco import _is_int, default_outer_spec, fused_sgd_hparams
from .federated_averaging import AveragingCommunicator
from .optim import OptimSpec, ensure_optim_spec

# DiLoCoStrategy's options without an island form, and the value that leaves each off
REFUSED = dict(outer_compression=None, outer_error_feedback=False, num_fragments=1, outer_delay=0, outer_mix=0)


def check_island_options(island_size, H, spec, kwargs):
    """The fused kernel's hyper-parameters for outer OptimSpec `spec`; ValueError for an
    island_size or H out of range, an outer optimizer without an island step, or an
    option of DiLoCoStrategy that has none."""
    if island_size is not None and (not _is_int(island_size) or island_size < 1):
        raise ValueError(f"island_size={island_size!r}: expected None or an integer >= 1")
    if not _is_int(H) or H < 1:
        raise ValueError(f"H={H!r}: expected an integer >= 1")
    hp = fused_sgd_hparams(spec)
    if hp is None:
        raise ValueError(f"IslandDiLoCoStrategy needs a plain torch.optim.SGD outer optimizer (the island outer step "
                         f"has no other update); got {spec.cls.__name__} with {dict(spec.kwargs or {})}")
    for name, off in REFUSED.items():
        v = kwargs.get(name, off)
        if isinstance(v, bool) != isinstance(off, bool) or v != off:
            raise ValueError(f"{name}={v!r} has no island form (no kernel for the combination); "
                             f"IslandDiLoCoStrategy takes only {name}={off!r}")
    return hp


def draw_islands(ranks, island_size):
    """Consecutive slices of island_size of the shuffled node ids, each ascending."""
    size = island_size if island_size is not None else len(ranks)
    return [sorted(ranks[i:i + size]) for i in range(0, len(ranks), size)]


class IslandDiLoCoCommunicator(AveragingCommunicator):
    """The island outer step as a communication module: AveragingCommunicator's partner
    draw, island sub-communicators and gather, then one ga_diloco_outer_islands launch
    on this node's own master and momentum (engine.DiLoCoOuterIslands, K_local = 1)."""

    def __init__(self, H: int = 100, island_size: Optional[int] = 2,
                 outer_optim: Optional[Union[str, OptimSpec]] = None, **kwargs):
        super().__init__(island_size=island_size, **kwargs)
        self.H = H
        self.outer_optim_spec = ensure_optim_spec(outer_optim, default_outer_spec())
        self._outer = None

    def _init_node(self, model, rank, num_nodes):
        s = self.strategy
        # what the strategy holds now: an option may have been set after construction
        self.H, self.island_size, self.outer_optim_spec = s.H, s.island_size, s.outer_optim_spec
        hp = check_island_options(self.island_size, self.H, self.outer_optim_spec, s.kwargs)
        a = s.arena
        # every node's master is rank 0's initial model (diloco.py:81-82)
        s.coll.broadcast_(a.flat, 0)
        self._outer = DiLoCoOuterIslands(s.coll, 1, a.n, a.device, a.dtype, **hp)
        self._outer.init_master(a.flat)
        s.engine = self._outer

    def communicate(self, model, rank: int, num_nodes: int, local_step: int) -> None:
        if not (local_step % self.H == 0 and local_step > 0):
            return
        a = self.strategy.arena
        a.check_bound()
        own = a.flat.view(1, -1)
        if num_nodes == 1:
            self._outer(own, [[0]], [[0]], own)
            return
        if self.island_size is not None and self.island_size < num_nodes:
            members = self._select_partners(rank, num_nodes)
        else:
            members, self._islands = set(range(num_nodes)), []
        rows, idx, _ = self._gather_island(members, num_nodes)
        me = sorted(members).index(rank)
        self._outer(rows, [idx], [[0 if i == me else -1 for i in range(len(idx))]], own)


class IslandDiLoCoStrategy(CommunicateOptimizeStrategy):
    def __init__(self, optim_spec: Optional[Union[str, OptimSpec]] = None,
                 outer_optim_spec: Optional[Union[str, OptimSpec]] = None, H: int = 100,
                 island_size: Optional[int] = 2, **kwargs):
        comm = IslandDiLoCoCommunicator(H=H, island_size=island_size, outer_optim=outer_optim_spec)
        check_island_options(island_size, H, comm.outer_optim_spec, kwargs)
        max_norm = kwargs.pop("max_norm", None)
        super().__init__(communication_modules=[comm], inner_optim=optim_spec, max_norm=max_norm, **kwargs)
        self.outer_optim_spec = comm.outer_optim_spec
        self.H = H
        self.island_size = island_size
        self.engine = None  # the node's DiLoCoOuterIslands once it is initialised (Strategy.placement_records)
