"""Flat step bodies: the strategy communication step over [K_local, ld]
replica sets, one kernel (plus at most one collective per exchange) per step.

Each engine is used by the Strategy API classes (K_local = 1: one simulated
node per process/GPU) and directly by the bench for batched-replica mode
(K_local > 1 simulated nodes on one GPU, reduced over K in-kernel before the
cross-GPU exchange).  World = number of processes in the collective; the
node count is K_total = world * K_local.

  MeanReduce   SimpleReduce grads, FedAvg params     strategy.py:128-142, federated_averaging.py:53-69
  DiLoCoOuter  fused outer SGD/Nesterov step        diloco.py:34-76
  DiLoCoOuterAdam  the same with an Adam/AdamW update  diloco.py:26-28
  DiLoCoOuterQuant  the SGD outer step on int8 / int4 block-quantised pseudo-gradients
  DiLoCoOuterStream  the SGD outer step sent at one step, merged `delay` steps later and mixed into the rows
  DiLoCoOuterIslands  the SGD outer step per node against its island's average, per-node master and momentum
  FragmentedOuter  Streaming DiLoCo's schedule: one outer engine per fragment of the arena (fragment_bounds)
  TorchOuter   any other outer optimizer: torch's, on an fp32 master
  Sparta       sparse average (Philox or mask)      sparta.py:24-44
  DeMoCodec    DCT encode/top-k + gather + decode   demo_impl/demo.py:142-209

Shared by them and by their callers in both modes: node_mean (row sum,
all-reduce, division by K_total) and place_replica_set (the probe-and-move of a
caller's [K, ld] set that MeanReduce and DiLoCoOuter each guard their own way).
"""
import math

import numpy as np
import torch

from . import ops
from .ops import TorchDraw
from .comm import DONE, Collective
from .demo_codec import DemoPlan


def _f32(x):
    return float(np.float32(x))


CHUNK_BYTES = 64 << 20  # pipeline chunk of the sharded exchange (RCCL stays at its large-message rate)
# ...and each rank's piece of a chunk (what one reduce-scatter delivers to it,
# one all-gather takes from it) at least this large, so wide worlds cut the
# arena into fewer, larger collectives (G=8: 128 MB chunks, 16 MB per rank).
PIECE_BYTES = 16 << 20


def chunk_bytes(world):
    return max(CHUNK_BYTES, world * PIECE_BYTES)
# Below this arena size the exchange is latency-bound: ONE all-reduce (RCCL's
# low-latency protocols, one launch) beats a reduce-scatter + shard kernel +
# all-gather, and the replicated local update costs microseconds.
SHARD_MIN_BYTES = 32 << 20


def default_shard(coll, n, dtype):
    """Shard the exchange (reduce-scatter -> shard kernel -> all-gather) when
    the collective is RCCL across processes and the arena is large enough to
    be bandwidth-bound; gloo (no reduce-scatter) and small arenas use one
    all-reduce."""
    esz = torch.empty((), dtype=dtype).element_size()
    return bool(coll.rccl and coll.exchange and n * esz >= SHARD_MIN_BYTES)


def node_mean(coll, reps, out, K_total):
    """out <- the mean of the rows of `reps` over all K_total nodes: the ascending
    fp32 sum of the local rows (ga_replica_mean), one all-reduce across the
    processes, true division by K_total (the reference's `/= num_nodes`)."""
    ops.replica_mean(reps, out, divisor=1.0)
    coll.all_reduce_(out)
    ops.replica_mean(out, out, divisor=float(K_total))


def place_replica_set(reps, probe, relocate_replicas, candidates, how):
    """Up to `candidates` fresh [K, ld] sets timed with `probe(set)` (the step's
    access pattern, every value written back unchanged) beside `reps` itself;
    when one beats it the caller's set moves there (relocate_replicas copies the
    contents and re-points the caller's views).  Returns (the set to use from
    now on, the buffer that holds it or None, the record)."""
    from . import placement
    K, ld = reps.shape

    def as_set(buf):
        return buf.tensor()[:K * ld].view(K, ld)

    best_buf, times = placement.choose(4 * K * ld, reps.device, lambda b: probe(as_set(b)), probe(reps), candidates,
                                       PLACEMENT_MAX_FRAC)
    best = 0
    if best_buf is not None:
        best = min(range(len(times)), key=lambda i: times[i])
        reps = as_set(best_buf)
        relocate_replicas(reps)
    return reps, best_buf, {"candidates": len(times), "probe_ms": [round(t, 4) for t in times], "chosen": best,
                            "how": how}


class ShardPlan:
    """Chunked reduce-scatter / all-gather plan over a flat arena of n elements.

    The arena is cut into C contiguous chunks (each a multiple of world*64
    elements); rank r owns the r-th 1/world slice of every chunk.  Its shard
    state (DiLoCo master/momentum, the reduce-scatter output) is the
    concatenation of those slices in chunk order.  Chunking lets the local
    kernels of chunk c+1 run while RCCL moves chunk c (software pipeline, see
    run())."""

    def __init__(self, n, world, rank, elem_bytes, chunks=None, align=64):
        unit = world * align
        if n % unit:
            raise ValueError(f"arena length {n} is not a multiple of world*{align} = {unit}")
        units = n // unit
        if chunks is None:
            chunks = max(1, -(-n * elem_bytes // chunk_bytes(world)))
        C = max(1, min(int(chunks), units))
        base, rem = divmod(units, C)
        self.n, self.world, self.rank = n, world, rank
        self.bounds, self.own, self.shard = [], [], []
        c0 = m0 = 0
        for i in range(C):
            cs = (base + (1 if i < rem else 0)) * unit
            pcs = cs // world
            self.bounds.append((c0, c0 + cs))
            self.own.append((c0 + rank * pcs, c0 + (rank + 1) * pcs))
            self.shard.append((m0, m0 + pcs))
            c0 += cs
            m0 += pcs
        self.per = m0

    def gather_shard(self, flat, out):
        """out <- this rank's slices of `flat` (shard layout)."""
        for (a, b), (m0, m1) in zip(self.own, self.shard):
            out[m0:m1].copy_(flat[a:b])

    def run(self, coll, reps, rs_out, shard_fn):
        """One exchange over replica set reps [K, >= n] (K >= 1):
          per chunk c:  reps[0,c] <- sum_k reps[k,c]          (K > 1, in place)
                        rs_out[shard c] <- reduce-scatter over ranks (RCCL)
                        shard_fn(rs_out[shard c], (m0, m1), reps[0, own c])
                        reps[0,c] <- all-gather of the owned slices (RCCL)
                        reps[1:,c] <- reps[0,c]                (K > 1)
        Issued with a lag of one chunk between the stages so the local
        kernels (current stream) overlap the collectives (RCCL stream):
        chunk c+1's sum runs while chunk c is reduce-scattered, chunk c-1's
        replica write-back while chunk c is all-gathered.  Work.wait() only
        orders the current stream after a collective; the host never blocks."""
        K = reps.shape[0]
        row0 = reps[0]
        rs_q, ag_q = [], []

        def finish_rs(i, w):
            w.wait()
            a, b = self.own[i]
            m0, m1 = self.shard[i]
            shard_fn(rs_out[m0:m1], (m0, m1), row0[a:b])
            c0, c1 = self.bounds[i]
            ag_q.append((i, coll.all_gather_into(row0[c0:c1], row0[a:b], async_op=True)))

        def finish_ag(i, w):
            w.wait()
            if K > 1:
                c0, c1 = self.bounds[i]
                ops.replica_mean(reps[0:1, c0:c1], reps[1:, c0:c1], divisor=1.0)

        for i, (c0, c1) in enumerate(self.bounds):
            if K > 1:
                ops.replica_mean(reps[:, c0:c1], reps[0:1, c0:c1], divisor=1.0)
            m0, m1 = self.shard[i]
            rs_q.append((i, coll.reduce_scatter(rs_out[m0:m1], row0[c0:c1], async_op=True)))
            if len(rs_q) > 1:
                finish_rs(*rs_q.pop(0))
            if len(ag_q) > 1:
                finish_ag(*ag_q.pop(0))
        while rs_q:
            finish_rs(*rs_q.pop(0))
        while ag_q:
            finish_ag(*ag_q.pop(0))


class MeanReduce:
    """Every replica <- (sum over all K_total nodes) / K_total.

    RCCL, world > 1: chunked reduce-scatter -> true division of the own slice
    -> all-gather (ShardPlan.run: the division touches 1/world of the arena
    and overlaps the exchange of the next chunk; the same bytes on the wire as
    one all-reduce).  gloo: all-reduce of the (locally pre-summed) arena."""

    def __init__(self, coll: Collective, K_local, n, device, dtype, shard=None, chunks=None, placement=True):
        self.coll, self.K_local, self.n = coll, int(K_local), int(n)
        self.K_total = coll.world * self.K_local
        # relocate_replicas(new): moves the caller's [K, ld] set into `new` (contents copied, the
        # caller's views re-pointed); set by the replica loop, None: the set stays where it is
        self.relocate_replicas = None
        self.place_opt = placement
        self.placement = None  # the placement probe's record
        self._placed_for = None
        self._reps_placed = None
        W, X = coll.world, coll.exchange
        self.shard = default_shard(coll, self.n, dtype) if shard is None else bool(shard and X)
        if self.shard:
            esz = torch.empty((), dtype=dtype).element_size()
            self.plan = ShardPlan(self.n, W, coll.rank, esz, chunks)
            self.rs_out = torch.empty(self.plan.per, device=device, dtype=dtype)
        self.sum = torch.empty(n, device=device, dtype=dtype) if (X and K_local > 1 and not self.shard) else None

    def _divide(self, rs_shard, m, own):
        ops.replica_mean(rs_shard, own, divisor=self.K_total)

    def _place(self, reps):
        """Once per replica set, single process: the in-place mean runs 1.49 or
        1.26 ms at GPT-2 124M x 8 depending on where the set sits physically
        (profiles/r05y_mean_placement.txt), so when the caller can move it
        (relocate_replicas) up to REPLICA_PLACEMENT_CANDIDATES fresh [K, ld] sets
        are timed with ga_probe_mean_placement (the step's access pattern, every
        value written back unchanged) and the set moves to the fastest when it
        beats its own time.  Returns the set to use from now on."""
        key = (reps.data_ptr(), reps.stride(0))
        if self._placed_for == key or self.relocate_replicas is None:
            return reps
        self._placed_for = key
        from . import placement
        ok, why = placement.policy(self.place_opt)
        if not ok:
            self.placement = {"placed": False, "why": why}
            return reps
        K, ld = reps.shape
        if (reps.device.type != "cuda" or reps.dtype != torch.float32 or not reps.is_contiguous() or K > 16
                or 4 * ld < SHARD_MIN_BYTES or self.n % 4 or ld % 4 or REPLICA_PLACEMENT_CANDIDATES < 2):
            return reps

        watch = placement.Stopwatch()
        reps, buf, self.placement = place_replica_set(
            reps, lambda t: placement.time_probe(lambda: ops.probe_mean_placement(t, self.n)), self.relocate_replicas,
            REPLICA_PLACEMENT_CANDIDATES, "the caller's replica set moved to the fastest of fresh [K, ld] allocations; "
                                          "candidate 0 = where it was")
        if buf is not None:
            self._reps_placed = buf
            self._placed_for = (reps.data_ptr(), reps.stride(0))
        watch.stamp(self.placement)
        return reps

    def __call__(self, reps):
        K, n = self.K_local, self.n
        if not self.coll.exchange:
            if K > 1:
                reps = self._place(reps)
                ops.replica_mean(reps, reps, n=n)
            return
        if self.shard:
            self.plan.run(self.coll, reps[:, :n], self.rs_out, self._divide)
            return
        if K == 1:
            self.coll.all_reduce_(reps[0, :n])
            ops.replica_mean(reps[0:1], reps[0:1], n=n, divisor=self.K_total)
        else:
            ops.replica_mean(reps, self.sum, n=n, divisor=1.0)
            self.coll.all_reduce_(self.sum)
            ops.replica_mean(self.sum, reps, n=n, divisor=self.K_total)


# physical master+momentum candidates (gym_amd.placement) timed against the replica set
# before the first outer step; the fastest is kept
PLACEMENT_CANDIDATES = 64
PLACEMENT_MAX_FRAC = 0.3  # of the free device memory the candidates may take at once
# fresh [K, ld] replica sets probed first when the caller lets the step move its replica
# set (DiLoCoOuter.relocate_replicas: the replica loop's ReplicaArena, the bench's set)
REPLICA_PLACEMENT_CANDIDATES = 12


class DiLoCoOuter:
    """Fused DiLoCo outer step.  With RCCL and world > 1 the master copy and
    the momentum are sharded: chunked reduce-scatter(sum) -> fused update of
    the own slice -> all-gather(params), software-pipelined over chunks
    (ShardPlan.run); the same bytes on the wire as the reference's all-reduce
    + broadcast, the outer-optimizer state / world per GPU."""

    def __init__(self, coll: Collective, K_local, n, device, dtype, lr=0.7, momentum=0.9, nesterov=True,
                 dampening=0.0, weight_decay=0.0, shard=None, chunks=None, placement=True):
        self.coll, self.K_local = coll, int(K_local)
        self.place_opt = placement  # False: never probe / move master+momentum (gym_amd.placement.policy)
        self.K_total = coll.world * self.K_local
        self.hp = dict(lr=lr, momentum=momentum, nesterov=nesterov, dampening=dampening, weight_decay=weight_decay)
        W, X = coll.world, coll.exchange
        self.n = int(n)
        self.shard = default_shard(coll, self.n, dtype) if shard is None else bool(shard and X)
        if self.shard:
            esz = torch.empty((), dtype=dtype).element_size()
            self.plan = ShardPlan(self.n, W, coll.rank, esz, chunks)
            self.per = self.plan.per
        else:
            self.plan = None
            self.per = self.n
        self._alloc_state(device)
        self.placement = None  # the placement probe's record (bench / DESIGN)
        self._placed_for = None
        self._placed = None  # the candidate buffer holding the state, when one was chosen
        # relocate_replicas(new): moves the caller's [K, ld] replica set into `new` (contents
        # copied, the caller's views re-pointed); None: the replica set stays where it is
        self.relocate_replicas = None
        self._reps_placed = None
        self.first = True
        self.dtype = dtype
        self.sum = torch.empty(n, device=device, dtype=dtype) if (X and not self.shard) else None
        self.rs_out = torch.empty(self.per, device=device, dtype=dtype) if self.shard else None
        self.launch_elems = []  # elements per ga_diloco_outer launch of the last step (bench roofline)

    def _alloc_state(self, device):
        # master and momentum in one allocation (a placement candidate, see _place)
        momentum = self.hp["momentum"]
        self._state = torch.zeros((2 if momentum != 0 else 1) * self.per, device=device, dtype=torch.float32)
        self.master = self._state[:self.per]
        self.mom = self._state[self.per:] if momentum != 0 else None

    def init_master(self, params_flat):
        """master <- the node's initial parameters (diloco.py:81-82)."""
        if self.shard:
            self.plan.gather_shard(params_flat, self.master)
        else:
            self.master.copy_(params_flat[:self.per])
        self.first = True

    def _outer(self, src, divisor, dst, m0=0, m1=None):
        h = self.hp
        m1 = self.per if m1 is None else m1
        mom = self.mom[m0:m1] if self.mom is not None else None
        ops.diloco_outer(src, self.master[m0:m1], mom, dst, m1 - m0, divisor, h["lr"], h["momentum"],
                         h["dampening"], h["weight_decay"], h["nesterov"], self.first)
        self.launch_elems.append(m1 - m0)

    def _outer_masked(self, reps, sparse_mask):
        h, n = self.hp, self.n
        ops.diloco_outer_masked(reps[:, :n], sparse_mask, self.master, self.mom, n, float(self.K_total),
                                self.K_total, h["lr"], h["momentum"], h["dampening"], h["weight_decay"],
                                h["nesterov"], self.first)
        self.launch_elems.append(n)

    def _outer_shard(self, rs_shard, m, own):
        self._outer(rs_shard, self.K_total, own, m[0], m[1])

    def _place(self, reps):
        """Choose the physical memory master / momentum live in, once per replica set.

        On MI355X the fused step's rate depends on where its 2K + 4 streams sit
        PHYSICALLY (gym_amd.placement: regions of several GB map to the HBM
        channels/banks differently; master/momentum in a region that maps like
        the replica set's make the step 1.88 instead of 1.57-1.65 ms at GPT-2
        124M x 8, and which one an allocation gets changes from process to
        process: the between-process spread of rounds 1-3).  So up to
        PLACEMENT_CANDIDATES fresh device allocations (one at a time, all held
        until the choice) are timed once against the live replica set with
        ga_probe_diloco_placement -- the step's exact access pattern, every value
        written back unchanged -- beside the ordinary allocation; the fastest
        keeps the state, the others are released.  ~0.2 s once; at most
        PLACEMENT_MAX_FRAC of the free memory at a time.

        The replica set's own region matters as much (r04i: with the replica set in a
        slow class no master placement reaches the fast one), so when the caller
        can move it (relocate_replicas) up to REPLICA_PLACEMENT_CANDIDATES fresh
        [K, ld] sets are probed first, against the ordinary master, and the replica
        set moves to the fastest when it beats its own.  Returns the replica set
        to use from now on."""
        key = (reps.data_ptr(), reps.stride(0))
        if self._placed_for == key:
            return reps
        self._placed_for = key
        per = self.per
        from . import placement
        ok, why = placement.policy(self.place_opt)
        if not ok:
            self.placement = {"placed": False, "why": why}
            return reps
        if (self.coll.exchange or reps.device.type != "cuda" or reps.dtype != torch.float32 or self.mom is None
                or reps.shape[0] > 16 or 4 * per < SHARD_MIN_BYTES or PLACEMENT_CANDIDATES < 2
                or reps.stride(1) != 1 or reps.stride(0) % 4 or per % 4):
            return reps
        rep_rec = None
        watch = placement.Stopwatch()
        if self.relocate_replicas is not None and REPLICA_PLACEMENT_CANDIDATES >= 2 and reps.is_contiguous():
            reps, rep_rec = self._place_replicas(reps, per)
            self._placed_for = (reps.data_ptr(), reps.stride(0))
        src = reps[:, :per]

        def probe_state(state):
            return placement.time_probe(lambda: ops.probe_diloco_placement(src, per, state[:per], state[per:2 * per]))

        best_buf, times = placement.choose(8 * per, reps.device, lambda b: probe_state(b.tensor()),
                                           probe_state(self._state), PLACEMENT_CANDIDATES, PLACEMENT_MAX_FRAC)
        best = 0
        if best_buf is not None:
            best = min(range(len(times)), key=lambda i: times[i])
            st = best_buf.tensor()[:2 * per]
            st.copy_(self._state)
            self._state, self._placed = st, best_buf
            self.master, self.mom = st[:per], st[per:]
        del src
        self.placement = {"candidates": len(times), "probe_ms": [round(t, 4) for t in times], "chosen": best,
                          "how": "master+momentum in fresh device allocations probed with the step's "
                                 "access pattern; candidate 0 = the ordinary allocation"}
        if rep_rec is not None:
            self.placement["replica_set"] = rep_rec
        watch.stamp(self.placement)  # both stages
        return reps

    def _place_replicas(self, reps, per):
        """Stage 1 of _place: fresh [K, ld] replica sets probed against the
        current master/momentum; the caller's set moves to the fastest one when
        it beats the set's own time (relocate_replicas copies the contents)."""
        from . import placement
        reps, buf, rec = place_replica_set(
            reps, lambda t: placement.time_probe(lambda: ops.probe_diloco_placement(t[:, :per], per, self.master,
                                                                                    self.mom)),
            self.relocate_replicas, REPLICA_PLACEMENT_CANDIDATES,
            "the caller's replica set moved to the fastest of fresh [K, ld] allocations "
            "(probed against the ordinary master); candidate 0 = where it was")
        if buf is not None:
            self._reps_placed = buf
        return reps, rec

    def __call__(self, reps, sparse_mask=None):
        """sparse_mask: packed int64 mask words (ops.sparta_pack_mask layout) of a
        SPARTA sparse average over all K_total nodes that this step also performs,
        just before the outer update, in the same pass (ga_diloco_outer_masked;
        bit-identical to Sparta followed by this step).  Single process only."""
        n = self.n
        self.launch_elems = []
        if sparse_mask is not None:
            if self.coll.exchange:
                raise ValueError("DiLoCoOuter: the masked outer step needs a local (no-exchange) step; run Sparta "
                                 "and the outer step one after the other")
            reps = self._place(reps)
            self._outer_masked(reps, sparse_mask)
        elif not self.coll.exchange:  # one kernel: read every replica, update, write every replica
            reps = self._place(reps)
            self._outer(reps[:, :n], self.K_total, reps[:, :n])
        elif not self.shard:  # gloo: all-reduce the sum, replicated update
            ops.replica_mean(reps, self.sum, n=n, divisor=1.0)
            self.coll.all_reduce_(self.sum)
            self._outer(self.sum, self.K_total, reps[:, :n])
        else:
            self.plan.run(self.coll, reps[:, :n], self.rs_out, self._outer_shard)
        self.first = False


class DiLoCoOuterAdam(DiLoCoOuter):
    """DiLoCoOuter for an Adam / AdamW outer optimizer: the same four branches
    (local in place, the masked boundary step, gloo, RCCL sharded through
    ShardPlan.run) around ga_diloco_outer_adam.  Master, exp_avg and exp_avg_sq
    are fp32 in one allocation of 3 * per (per = n / world when sharded); the
    engine counts the outer steps (t) and hands the kernel torch's bias
    corrections, computed in Python doubles as ArenaAdam does.  `mom` is None
    and `hp` holds Adam's hyper-parameters; there is no placement search (the
    probe kernel models two state streams, this step has three)."""

    def __init__(self, coll: Collective, K_local, n, device, dtype, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, decoupled=False, shard=None, chunks=None, placement=True):
        super().__init__(coll, K_local, n, device, dtype, lr=lr, momentum=0.0, nesterov=False,
                         weight_decay=weight_decay, shard=shard, chunks=chunks, placement=placement)
        self.hp = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                       weight_decay=float(weight_decay), decoupled=bool(decoupled))
        self.t = 0  # outer steps taken

    def _alloc_state(self, device):
        per = self.per
        self._state = torch.zeros(3 * per, device=device, dtype=torch.float32)
        self.master, self.exp_avg, self.exp_avg_sq = (self._state[i * per:(i + 1) * per] for i in range(3))
        self.mom = None

    def init_master(self, params_flat):
        super().init_master(params_flat)
        self.t = 0
        self._state[self.per:].zero_()

    def scalars(self, t):
        """ga_diloco_outer_adam's scalars at outer step t (torch's _single_tensor_adam)."""
        h = self.hp
        lr, (b1, b2), wd = h["lr"], h["betas"], h["weight_decay"]
        return dict(lerp_w=1 - b1, beta2=b2, one_m_beta2=1 - b2, eps=h["eps"],
                    wd_factor=(1 - lr * wd) if (h["decoupled"] and wd != 0) else 1.0,
                    l2_wd=wd if (not h["decoupled"] and wd != 0) else 0.0,
                    step_size=-(lr / (1 - b1 ** t)), bc2_sqrt=math.sqrt(1 - b2 ** t))

    def _place(self, reps):
        if self.placement is None:
            self.placement = {"placed": False, "why": "no search for the Adam outer step (three state streams)"}
        return reps

    def _outer(self, src, divisor, dst, m0=0, m1=None):
        m1 = self.per if m1 is None else m1
        ops.diloco_outer_adam(src, self.master[m0:m1], self.exp_avg[m0:m1], self.exp_avg_sq[m0:m1], dst, m1 - m0,
                              divisor, **self._scalars)
        self.launch_elems.append(m1 - m0)

    def _outer_masked(self, reps, sparse_mask):
        n = self.n
        ops.diloco_outer_adam_masked(reps[:, :n], sparse_mask, self.master, self.exp_avg, self.exp_avg_sq, n,
                                     float(self.K_total), self.K_total, **self._scalars)
        self.launch_elems.append(n)

    def __call__(self, reps, sparse_mask=None):
        self._scalars = self.scalars(self.t + 1)
        super().__call__(reps, sparse_mask)
        self.t += 1


class TorchOuter:
    """DiLoCo's outer step for an outer OptimSpec without a fused kernel
    (diloco.py:26-28, 34-49, 66-74), with DiLoCoOuter's call surface: torch's
    optimizer on an fp32 master of the node's start (replicated on every
    process), fed the node average (node_mean); every row takes the master."""

    relocate_replicas = None  # accepted as on DiLoCoOuter; nothing here depends on where the set sits

    def __init__(self, coll: Collective, K_local, n, device, dtype, spec):
        self.coll, self.spec = coll, spec
        self.K_total = coll.world * int(K_local)
        self.avg = torch.empty(n, device=device, dtype=dtype)
        self.master = self.optimizer = None

    def init_master(self, params_flat):
        self.master = torch.nn.Parameter(params_flat.detach().float().clone())
        self.optimizer = self.spec.build([self.master])

    @torch.no_grad()
    def __call__(self, reps, sparse_mask=None):
        if sparse_mask is not None:
            raise ValueError("TorchOuter: no one-pass masked outer step; run Sparta and the outer step one after "
                             "the other")
        node_mean(self.coll, reps, self.avg, self.K_total)
        self.optimizer.zero_grad()
        self.master.grad = self.master.detach() - self.avg.float()
        self.optimizer.step()
        reps.copy_(self.master.detach())  # broadcast over the rows


QUANT_BITS = {"int8": 8, "int4": 4}  # the outer_compression strings of the strategies


class DiLoCoOuterQuant:
    """DiLoCo's outer step (SGD family) on int8 / int4 block-quantised
    pseudo-gradients, with DiLoCoOuter's call surface.

    Every node quantises its own pseudo-gradient master - x_k in 256-element
    blocks with one fp32 scale each (ga_quant_encode), the payload rows are
    all-gathered in node order, and one launch per process decodes all K_total
    rows in ascending node order, averages them and takes the outer update
    (ga_diloco_outer_dequant).  Every process decodes the same bytes in the same
    order, so all nodes end bit-identical without a broadcast.

    Master and momentum are fp32 and REPLICATED on every process, not sharded as
    DiLoCoOuter's: a rank needs the whole master to form its own delta (8 B per
    parameter per rank).  error_feedback keeps a [K_local, n] fp32 residual: what
    quantisation dropped from a node's delta is added to its next one.  No
    placement search and no masked (SPARTA boundary) step."""

    def __init__(self, coll: Collective, K_local, n, device, dtype, bits=8, error_feedback=False, lr=0.7,
                 momentum=0.9, nesterov=True, dampening=0.0, weight_decay=0.0, placement=True):
        if bits not in (4, 8):
            raise ValueError(f"DiLoCoOuterQuant: bits={bits!r} is not 4 or 8")
        self.coll, self.K_local, self.n, self.bits = coll, int(K_local), int(n), int(bits)
        self.K_total = coll.world * self.K_local
        self.hp = dict(lr=lr, momentum=momentum, nesterov=nesterov, dampening=dampening, weight_decay=weight_decay)
        self.shard, self.per, self.dtype = False, self.n, dtype
        self._state = torch.zeros((2 if momentum != 0 else 1) * self.n, device=device, dtype=torch.float32)
        self.master = self._state[:self.n]
        self.mom = self._state[self.n:] if momentum != 0 else None
        self.residual = (torch.zeros(self.K_local, self.n, device=device, dtype=torch.float32)
                         if error_feedback else None)
        self.payload_bytes_per_node = ops.quant_row_bytes(self.n, self.bits)
        self.payload = torch.zeros(self.K_total, self.payload_bytes_per_node, device=device, dtype=torch.uint8)
        self.placement = {"placed": False, "why": "no search for the quantised outer step"}
        self.relocate_replicas = None  # accepted as on DiLoCoOuter; the set stays where it is
        self.first = True
        self.launch_elems = []  # elements per ga_diloco_outer_dequant launch of the last step

    def init_master(self, params_flat):
        """master <- the node's initial parameters (diloco.py:81-82); no error carried over."""
        self.master.copy_(params_flat[:self.n])
        if self.residual is not None:
            self.residual.zero_()
        self.first = True

    def __call__(self, reps, sparse_mask=None):
        if sparse_mask is not None:
            raise ValueError("DiLoCoOuterQuant: no one-pass masked outer step; run Sparta and the outer step one "
                             "after the other")
        n, K, h = self.n, self.K_local, self.hp
        a = self.coll.rank * K
        own = self.payload[a:a + K]
        ops.quant_encode(reps[:, :n], self.master, self.residual, own, n, self.bits)
        if self.coll.exchange:
            self.coll.all_gather_into(self.payload.view(-1), own.view(-1))
        ops.diloco_outer_dequant(self.payload, self.master, self.mom, reps[:, :n], n, self.bits, self.K_total,
                                 h["lr"], h["momentum"], h["dampening"], h["weight_decay"], h["nesterov"], self.first)
        self.launch_elems = [n]
        self.first = False


class DiLoCoOuterStream:
    """Streaming DiLoCo's outer step (SGD family) for one fragment: the exchange
    is sent at one step and its result merged `delay` inner steps later, mixed
    into the live rows instead of overwriting them:
        x_k <- mix * x_k + (1 - mix) * master        (ga_diloco_outer_merge)

    send(reps) stages the ascending fp32 sum of the local rows in one row of the
    arena's dtype and starts its all-reduce (async under RCCL: the collective runs
    on RCCL's stream under the next `delay` inner steps; gloo completes it at
    once, with the same numerics).  receive(reps) waits for it and makes one merge
    launch: the outer update on the staged sum over K_total, then the blend into
    every live row.  Calling the engine is send then receive; with no exchange and
    no delay that is one in-place launch over the rows and no staging row.

    Master and momentum are fp32 and REPLICATED on every process, not sharded as
    DiLoCoOuter's (8 B per parameter per rank, plus the staging row; `shard` and
    `chunks` are accepted as on DiLoCoOuter and ignored).  No placement search and no
    masked (SPARTA boundary) step."""

    def __init__(self, coll: Collective, K_local, n, device, dtype, lr=0.7, momentum=0.9, nesterov=True,
                 dampening=0.0, weight_decay=0.0, delay=0, mix=0.0, shard=None, chunks=None, placement=True):
        if int(delay) != delay or delay < 0:
            raise ValueError(f"DiLoCoOuterStream: delay={delay!r} is not an integer >= 0")
        if not 0.0 <= float(mix) < 1.0:
            raise ValueError(f"DiLoCoOuterStream: mix={mix!r} is not in [0, 1)")
        self.coll, self.K_local, self.n = coll, int(K_local), int(n)
        self.K_total = coll.world * self.K_local
        self.delay, self.mix = int(delay), float(mix)
        self.hp = dict(lr=lr, momentum=momentum, nesterov=nesterov, dampening=dampening, weight_decay=weight_decay)
        self.shard, self.per, self.dtype = False, self.n, dtype
        self._state = torch.zeros((2 if momentum != 0 else 1) * self.n, device=device, dtype=torch.float32)
        self.master = self._state[:self.n]
        self.mom = self._state[self.n:] if momentum != 0 else None
        self.staged = bool(coll.exchange or self.delay > 0)
        self.stage = torch.zeros(self.n, device=device, dtype=dtype) if self.staged else None
        self._work = None  # the handle of the exchange in flight
        self.placement = {"placed": False, "why": "no search for the streaming outer step"}
        self.relocate_replicas = None  # accepted as on DiLoCoOuter; the set stays where it is
        self.first = True
        self.launch_elems = []  # elements per ga_diloco_outer_merge launch of the last receive

    def init_master(self, params_flat):
        """master <- the node's initial parameters (diloco.py:81-82); nothing in flight."""
        self.cancel()
        self.master.copy_(params_flat[:self.n])
        self.first = True

    def send(self, reps):
        if not self.staged:
            return
        ops.replica_mean(reps[:, :self.n], self.stage, n=self.n, divisor=1.0)
        self._work = self.coll.all_reduce_(self.stage, async_op=True)

    def receive(self, reps):
        n, h = self.n, self.hp
        if self.staged:
            if self._work is None:
                raise RuntimeError("DiLoCoOuterStream.receive: nothing was sent")
            self._work.wait()
            self._work = None
            src = self.stage
        else:
            src = reps[:, :n]
        ops.diloco_outer_merge(src, self.master, self.mom, reps[:, :n], n, float(self.K_total), h["lr"],
                               h["momentum"], h["dampening"], h["weight_decay"], h["nesterov"], self.first, self.mix)
        self.launch_elems = [n]
        self.first = False

    def cancel(self):
        """Wait for an exchange in flight and drop its result."""
        if self._work is not None:
            self._work.wait()
            self._work = None

    def __call__(self, reps, sparse_mask=None):
        if sparse_mask is not None:
            raise ValueError("DiLoCoOuterStream: no one-pass masked outer step; run Sparta and the outer step one "
                             "after the other")
        self.send(reps)
        self.receive(reps)


class DiLoCoOuterIslands:
    """The island outer step (SGD family): every local node takes DiLoCo's outer
    update against the average of its island, on a master and a momentum row of its
    own (ga_diloco_outer_islands).

    The caller draws the islands and brings their rows together (FedAvg's draw and
    gather: strategy.island_diloco, replica.ReplicaRunner); a call makes ONE launch
    for the round over exactly the islands that have a local member:
        engine(src, islands, slots, x)
    src [S, >= n] holds the gathered rows, islands[j] the ascending rows of island j,
    slots[j][i] the local row (of master, momentum and x) of member islands[j][i] or
    -1 for a member hosted by another process, x [K_local, >= n] the local nodes'
    live rows (src itself for the in-place step of one process).

    Master and momentum are fp32 and live PER NODE, [K_local, n] each (8 B per
    parameter and node; DiLoCoOuter keeps one sharded copy for all nodes).  All nodes
    take every round, so `first` is one flag.  No placement search, no masked (SPARTA
    boundary) step, no exchange of its own (`coll` is kept for the record only)."""

    def __init__(self, coll: Collective, K_local, n, device, dtype, lr=0.7, momentum=0.9, nesterov=True,
                 dampening=0.0, weight_decay=0.0):
        self.coll, self.K_local, self.n, self.dtype = coll, int(K_local), int(n), dtype
        self.hp = dict(lr=lr, momentum=momentum, nesterov=nesterov, dampening=dampening, weight_decay=weight_decay)
        self.master = torch.zeros(self.K_local, self.n, device=device, dtype=torch.float32)
        self.mom = (torch.zeros(self.K_local, self.n, device=device, dtype=torch.float32)
                    if momentum != 0 else None)
        self.placement = {"placed": False, "why": "no search for the island outer step"}
        self.first = True
        self.launch_elems = []  # elements per row of each ga_diloco_outer_islands launch of the last round

    def init_master(self, params_flat):
        """Every node's master <- node 0's initial parameters (diloco.py:81-82)."""
        self.master.copy_(params_flat[:self.n].to(torch.float32).expand(self.K_local, self.n))
        self.first = True

    def __call__(self, src, islands, slots, x):
        local = [(list(isl), list(sl)) for isl, sl in zip(islands, slots) if any(v >= 0 for v in sl)]
        if not local:
            raise ValueError("DiLoCoOuterIslands: no island has a local member")
        n, h = self.n, self.hp
        ops.diloco_outer_islands(src[:, :n], [i for i, _ in local], [s for _, s in local], self.master, self.mom,
                                 x[:, :n], n, h["lr"], h["momentum"], h["dampening"], h["weight_decay"],
                                 h["nesterov"], self.first)
        self.launch_elems = [n]
        self.first = False


def fragment_bounds(offsets, n, F, unit):
    """[c_0 = 0, c_1, ..., c_F = n]: the arena cut into F fragments at tensor starts.
    For 0 < f < F, c_f is the start offset of the tensor nearest to f * n / F (a
    tie goes to the lower offset), rounded down to a multiple of `unit` -- the
    arena's padding unit, 512 * world elements, so that shard plans, 256-element
    quantisation blocks and 16-byte vector access hold on every fragment.  A cut
    that rounding moves inside a tensor is harmless: the outer update is
    element-wise.  ValueError when the bounds are not strictly increasing."""
    n, F, unit = int(n), int(F), int(unit)
    offs = sorted(int(o) for o in offsets)
    if F < 1 or unit < 1 or not offs:
        raise ValueError(f"fragment_bounds: F={F}, unit={unit}, {len(offs)} tensors")
    bounds = [0]
    for f in range(1, F):
        # |o - f n / F| compared exactly, as |o F - f n|
        near = min(offs, key=lambda o: (abs(o * F - f * n), o))
        bounds.append(near // unit * unit)
    bounds.append(n)
    if any(b <= a for a, b in zip(bounds, bounds[1:])):
        raise ValueError(f"num_fragments too large for this model: {F} fragments of {n} elements in units of {unit} "
                         f"cut at {bounds}")
    return bounds


class FragmentedOuter:
    """Streaming DiLoCo's schedule over F fragments [a_f, b_f) of the arena, one
    outer engine per fragment.  Fragment f takes its outer step when
        local_step > 0 and (local_step + (f * H) // F) % H == 0
    so every fragment fires once per H steps, staggered by H / F, and an outer
    event moves about n / F elements instead of n (fragment 0, and F = 1, keep
    DiLoCo's steps).  With delay == 0 the fragment's engine is called; otherwise
    it sends at that step and receives -- the merge -- `delay` steps later.

    step(reps, local_step) is called on every step, after the inner optimizer.
    finish() waits for the exchanges in flight and discards the merges still
    pending: the parameters are left as the inner steps made them."""

    def __init__(self, engines, bounds, H, delay=0):
        self.engines, self.bounds = list(engines), [int(b) for b in bounds]
        self.H, self.delay = int(H), int(delay)
        F = len(self.engines)
        if F < 1 or len(self.bounds) != F + 1:
            raise ValueError(f"FragmentedOuter: {F} engines for {len(self.bounds)} bounds")
        if not 0 <= self.delay < self.H:
            raise ValueError(f"FragmentedOuter: delay={delay!r} is not in [0, H = {H})")
        if self.delay and not all(hasattr(e, "send") and hasattr(e, "receive") for e in self.engines):
            raise ValueError("FragmentedOuter: a delay needs engines with send / receive (DiLoCoOuterStream)")
        self.due = [None] * F  # the step at which fragment f's pending merge lands
        self.launch_elems = []  # of the last step() call
        self.relocate_replicas = None  # accepted as on DiLoCoOuter; the set stays where it is
        self.placement = {"placed": False, "why": "no search for a fragmented outer step", "fragments": F,
                          "bounds": list(self.bounds)}

    @property
    def F(self):
        return len(self.engines)

    def fires(self, f, local_step):
        return local_step > 0 and (local_step + (f * self.H) // self.F) % self.H == 0

    def init_master(self, params_flat):
        self.due = [None] * self.F
        for f, eng in enumerate(self.engines):
            eng.init_master(params_flat[self.bounds[f]:self.bounds[f + 1]])

    def step(self, reps, local_step):
        self.launch_elems = []
        for f, eng in enumerate(self.engines):
            view = reps[:, self.bounds[f]:self.bounds[f + 1]]
            if self.due[f] is not None and self.due[f] <= local_step:
                eng.receive(view)
                self.due[f] = None
                self.launch_elems += eng.launch_elems
            if self.fires(f, local_step):
                if self.delay == 0:
                    eng(view)
                    self.launch_elems += eng.launch_elems
                else:
                    eng.send(view)
                    self.due[f] = local_step + self.delay

    def finish(self):
        for f, eng in enumerate(self.engines):
            if self.due[f] is not None:
                eng.cancel()
                self.due[f] = None


def sparta_capacity(n, p):
    """Packed-value capacity for a Philox draw of n elements at rate p: mean +
    16 sigma + 1024 (overflow is flagged on the device and raised by check())."""
    mu = n * p
    return int(min(n, math.ceil(mu + 16.0 * math.sqrt(max(mu * (1 - p), 1.0)) + 1024)))


class Sparta:
    """SPARTA sparse averaging over the whole arena in one select/gather, one
    all-reduce of the packed values, one scatter.  layout="rows": the replica
    set is [K_local, ld] (the training loop's layout); "elem": [n, K_local]
    element-major, where one element's K replicas share a line (batched-replica
    sets built for the step alone, e.g. the bench's configs[3])."""

    def __init__(self, coll: Collective, K_local, n, device, dtype, p, layout="rows"):
        self.coll, self.K_local, self.n, self.p = coll, int(K_local), int(n), float(p)
        self.layout = layout
        self.K_total = coll.world * self.K_local
        self.device, self.dtype = torch.device(device), dtype
        self.cap = sparta_capacity(n, self.p)
        self.idx = torch.empty(self.cap, dtype=torch.int32, device=device)
        self.vals = torch.empty(self.cap, dtype=dtype, device=device)
        self.count = torch.zeros(2, dtype=torch.int64, device=device)
        self.work = ops.sparta_workspace(n, device)
        # overflow flags read back asynchronously: two pinned host slots used in turn, each
        # with the event of the step that filled it (see check / _poll)
        self._flag_host = [torch.zeros(2, dtype=torch.int64, pin_memory=torch.cuda.is_available()) for _ in range(2)]
        self._flag_slot = 0
        self._pending = []  # [(event, host slot)] of steps not checked yet, oldest first
        self.bits = None  # packed mask broadcast buffer (mask mode with an exchange)

    def _ensure_cap(self, cap):
        if cap > self.cap:
            self.cap = cap
            self.idx = torch.empty(cap, dtype=torch.int32, device=self.device)
            self.vals = torch.empty(cap, dtype=self.dtype, device=self.device)

    @staticmethod
    def pack(mask, bits):
        """bits <- the uint8 mask arena `mask` as one bit per element (ga_sparta_pack_mask)."""
        ops.sparta_pack_mask(mask, mask.numel(), bits)
        return bits

    def check(self):
        """Raise if an earlier Philox step selected more than the capacity.

        The capacity is mean + 16 sigma + 1024 of the Binomial(n, p) count, so
        an overflow has probability < 1e-50 per step; the flag is still read
        back (asynchronously, no host sync in the step) and raised two steps
        later, or by an explicit check() -- the strategies call it when
        training ends, so even the last step is covered."""
        self._poll(0)

    def _poll(self, keep):
        """Check the oldest pending flags until at most `keep` remain.  A step
        polls with keep=1: it waits only for the step before the previous one,
        which the GPU has finished while it ran the previous one, so the host
        never waits on the GPU mid-stream (with keep=0 every step waited for the
        previous step's kernels and its own launches ran on an idle GPU)."""
        while len(self._pending) > keep:
            ev, hb = self._pending.pop(0)
            ev.synchronize()
            if int(hb[1]) != 0:
                self._pending.clear()
                raise RuntimeError(f"SPARTA: {int(hb[0])} elements selected > capacity {self.cap}")

    def __call__(self, reps, seed=0, iteration=0, mask=None, skip=None, mask_cap=None, mask_shared=False):
        """mask: this process's uint8/bool mask arena (the reference selector's
        draws), or its packed int64 words, or None for the Philox stream.  With an exchange, rank 0's mask
        wins (sparta.py:32-37): it is packed to one bit per element and
        broadcast (n/8 bytes; every rank's own draw is overwritten).
        mask_cap: a bound on the selected count that holds on every rank (e.g.
        sparta_capacity for Bernoulli masks): no host sync for the exact count,
        overflow flagged on the device as in Philox mode.  None: the exact
        count is read back (any selector).
        mask_shared: the mask is already rank 0's on every rank (the fused
        reference draw from rank 0's broadcast generator state): no mask
        broadcast."""
        n = self.n
        cnt = None
        if isinstance(mask, TorchDraw):  # the reference draw, computed inside the average kernel
            if self.coll.exchange:
                raise ValueError("Sparta: an in-kernel reference draw needs a local (no-exchange) step")
            ops.sparta_average_local(reps, n, float(self.K_total), mask=mask, layout=self.layout)
            return
        if mask is not None and mask.dtype == torch.int64:  # already packed (the fused reference draw)
            if mask_cap is None:
                raise ValueError("Sparta: a packed mask needs mask_cap")
            if self.coll.exchange and not mask_shared:
                self.coll.broadcast_(mask[:ops.sparta_mask_words(n)], 0)
        elif mask is not None and self.coll.exchange:
            words = ops.sparta_mask_words(n)
            if self.bits is None:  # the packed words + rank 0's selected count in the last word
                self.bits = torch.empty(words + 1, dtype=torch.int64, device=self.device)
            ops.sparta_pack_mask(mask, n, self.bits)
            if mask_cap is None:
                self.bits[words:].copy_(mask[:n].sum(dtype=torch.int64).view(1))
            self.coll.broadcast_(self.bits, 0)
            mask = self.bits[:words]
            if mask_cap is None:
                cnt = self.bits[words]
        if mask is not None and mask_cap is None:  # exact count known from the mask
            cnt = mask[:n].sum() if cnt is None else cnt
            cap = max(1, int(cnt.item()))
            self._ensure_cap(cap)
            cap_used = cap
        else:
            if mask is not None:
                self._ensure_cap(int(mask_cap))
            self._poll(1)
            cap_used = self.cap
        if not self.coll.exchange:  # every node is a local replica: one fused pass, no exchange
            ops.sparta_average_local(reps, n, float(self.K_total), mask=mask, seed=seed, iteration=iteration,
                                     p=self.p, skip=skip, layout=self.layout)
            return
        ops.sparta_select(reps, n, cap_used, self.idx, self.vals, self.count, self.work, mask=mask, seed=seed,
                          iteration=iteration, p=self.p, skip=skip, layout=self.layout)
        self.coll.all_reduce_(self.vals[:cap_used])
        ops.sparta_scatter(self.vals, self.idx, self.count, cap_used, float(self.K_total), reps, layout=self.layout)
        if mask is None or mask_cap is not None:  # overflow flag read back asynchronously, checked next step
            hb = self._flag_host[self._flag_slot]
            self._flag_slot ^= 1
            hb.copy_(self.count, non_blocking=True)
            if self.device.type == "cuda":
                ev = torch.cuda.Event()
                ev.record()
                self._pending.append((ev, hb))
            elif int(hb[1]) != 0:
                raise RuntimeError(f"SPARTA: {int(hb[0])} elements selected > capacity {self.cap}")


class DeMoCodec:
    """DeMo step: encode every replica's delta (DCT + top-k + residual), one
    all-gather of the packed payloads, decode + sign-SGD applied to every
    replica.  Payload per node: int32 idx[M] then fp32 val[M]."""

    def __init__(self, coll: Collective, K_local, layout, device, chunk=64, topk=32, bf16_transform="fp32"):
        self.coll, self.K_local = coll, int(K_local)
        self.K_total = coll.world * self.K_local
        self.plan = DemoPlan(layout, chunk=chunk, topk=topk, bf16_transform=bf16_transform).to(device)
        M = self.plan.M
        self.payload = torch.zeros(self.K_local, 2 * M, dtype=torch.int32, device=device)
        self.gathered = (torch.zeros(self.K_total, 2 * M, dtype=torch.int32, device=device)
                         if coll.exchange else self.payload)

    def encode(self, P, G, D, lr, decay, weight_decay):
        wdf = _f32(1.0 - lr * weight_decay) if weight_decay != 0.0 else 1.0
        ops.demo_encode(self.plan, P, G, D, self.payload, _f32(lr), _f32(decay), wdf)

    def exchange(self, all_gather=None):
        if not self.coll.exchange:
            return
        if all_gather is None:
            self.coll.all_gather_into(self.gathered.view(-1), self.payload.view(-1))
        else:  # a user-supplied list-style all_gather (DeMo(custom_all_gather=...))
            parts = list(self.gathered.view(self.coll.world, -1).unbind(0))
            h = all_gather(parts, self.payload.view(-1), group=self.coll.group, async_op=True)
            if h is not None and hasattr(h, "wait"):
                h.wait()

    def decode(self, P, G, lr):
        ops.demo_decode(self.plan, self.gathered, P, G, _f32(lr))

    def place(self, P, G, D, lr, decay=0.999):
        """Placement of the step's parameters, gradient and delta (see
        place_demo_step): the decode probed with this codec's last gathered
        payload, the encode (the step's lr and decay: the chunks take the same
        top-k path as in the step) into a scratch payload."""
        scratch = torch.empty_like(self.payload)
        return place_demo_step(
            lambda p, g, d: ops.demo_encode(self.plan, p, g, d, scratch, _f32(lr), _f32(decay), 1.0),
            lambda p, g: ops.demo_decode(self.plan, self.gathered, p, g, 0.0), P, G, D)

    def __call__(self, P, G, D, lr, decay=0.999, weight_decay=0.0, all_gather=None):
        self.encode(P, G, D, lr, decay, weight_decay)
        self.exchange(all_gather)
        self.decode(P, G, lr)


import os as _os

# tensor groups of the pipelined DeMo exchange (RCCL, world > 1); GA_DEMO_PIECES overrides
DEMO_PIECES = int(_os.environ.get("GA_DEMO_PIECES", "2"))


# DeMo step placement: fresh allocations probed per buffer
DEMO_PLACEMENT_CANDIDATES = 32
DEMO_PLACEMENT_MAX_FRAC = 0.3
DEMO_PLACEMENT_MIN_BYTES = 64 << 20


def place_demo_step(encode, decode, P, G, D):
    """Where the DeMo step's parameters, gradient and delta sit physically sets
    its rate the way master/momentum set the DiLoCo step's (GPT-2 350M 8-source
    decode: 1.13 ms in ordinary allocations, 1.00 ms with either buffer in a
    fast candidate, profiles/r04q_demo_decode_placement.txt).  `encode(P', G',
    D')` and `decode(P', G')` are the step's kernels on any such buffers (the
    decode at lr = 0 with the last gathered payload, the encode with the step's
    lr into a scratch payload); gym_amd.placement.place_each probes up to
    DEMO_PLACEMENT_CANDIDATES fresh allocations for G, then P, then D, each with
    the others where they are by then, restores all three, and returns
    ((buffer or None for P, G, D), (the P, G, D to use from now on), a record),
    or (None, None, None) when the buffers are not worth it."""
    from . import placement
    if (P.device.type != "cuda" or not (P.shape == G.shape == D.shape)
            or not (P.is_contiguous() and G.is_contiguous() and D.is_contiguous())
            or 3 * P.numel() * P.element_size() < DEMO_PLACEMENT_MIN_BYTES or DEMO_PLACEMENT_CANDIDATES < 2):
        return None, None, None

    def run(g, p, d):
        encode(p, g, d)
        decode(p, g)
    watch = placement.Stopwatch()
    try:  # only the snapshots can run out of memory before anything is touched (candidates: choose)
        (bg, bp, bd), (g2, p2, d2), stages = placement.place_each([G, P, D], run, DEMO_PLACEMENT_CANDIDATES,
                                                                  DEMO_PLACEMENT_MAX_FRAC)
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None, None, {"placed": False, "why": "no memory for the snapshots"}
    rec = {"what": "DeMo gradient, then parameters, then delta, each in the fresh device allocation the step's "
                   "encode + decode run fastest on (probed with the others where they are by then)",
           "ordinary_ms": round(stages[0], 4), "grad_placed_ms": round(stages[1], 4),
           "param_placed_ms": round(stages[2], 4), "delta_placed_ms": round(stages[3], 4),
           "placed": [b is not None for b in (bg, bp, bd)], "candidates_per_buffer": DEMO_PLACEMENT_CANDIDATES}
    return (bp, bg, bd), (p2, g2, d2), watch.stamp(rec)


def demo_codec(coll: Collective, K_local, layout, device, chunk=64, topk=32, bf16_transform="fp32"):
    """The DeMo codec an exchange should use: pipelined over DEMO_PIECES tensor
    groups when the all-gather is an async RCCL collective across processes,
    else one encode -> all-gather -> decode."""
    if coll.rccl and coll.exchange and DEMO_PIECES > 1 and len(layout.numels) > 1:
        return PipelinedDeMoCodec(coll, K_local, layout, device, chunk=chunk, topk=topk, pieces=DEMO_PIECES,
                                  bf16_transform=bf16_transform)
    return DeMoCodec(coll, K_local, layout, device, chunk=chunk, topk=topk, bf16_transform=bf16_transform)


def split_tensors(numels, pieces):
    """Contiguous groups of tensor indices with about equal element counts
    (at most `pieces` groups, none empty)."""
    total = sum(numels)
    groups, cur, acc = [], [], 0
    for i, n in enumerate(numels):
        cur.append(i)
        acc += n
        if len(groups) < pieces - 1 and acc * pieces >= total * (len(groups) + 1):
            groups.append(cur)
            cur = []
    if cur:
        groups.append(cur)
    return groups


class PipelinedDeMoCodec:
    """DeMoCodec over P groups of whole tensors, software-pipelined across the
    exchange: piece p's all-gather (RCCL, async) runs while piece p+1 is
    encoded and piece p-1 decoded, so at G GPUs the ~(G-1)/G of the payload
    crossing xGMI hides behind the codec kernels.  Each piece is a codec of its
    own over a subset of the tensors (same arena offsets, its own payload
    [idx m_p | val m_p]); per chunk the arithmetic, the entries and the source
    order are the ones of the unpipelined codec, so results are identical.
    Same call signature as DeMoCodec.__call__ (no custom all_gather)."""

    def __init__(self, coll: Collective, K_local, layout, device, chunk=64, topk=32, pieces=None,
                 bf16_transform="fp32"):
        self.coll = coll
        pieces = DEMO_PIECES if pieces is None else pieces
        groups = split_tensors(layout.numels, max(1, int(pieces)))
        self.codecs = [DeMoCodec(coll, K_local, layout.subset(g), device, chunk=chunk, topk=topk,
                                 bf16_transform=bf16_transform) for g in groups]
        # every piece runs the kernel family the whole plan would (the wave-per-chunk
        # kernels only if every chunk of the model qualifies), so the results match
        if not DemoPlan(layout, chunk=chunk, topk=topk, bf16_transform=bf16_transform).wave_encode:
            for c in self.codecs:
                c.plan.wave_encode = False
        self.M = sum(c.plan.M for c in self.codecs)

    def reference_bytes(self, val_itemsize=4):
        return sum(c.plan.reference_bytes(val_itemsize) for c in self.codecs)

    def place(self, P, G, D, lr, decay=0.999):
        """place_demo_step over every piece's encode and decode (each piece's last gathered payload)."""
        scratch = [torch.empty_like(c.payload) for c in self.codecs]

        def encode(p, g, d):
            for c, sc in zip(self.codecs, scratch):
                ops.demo_encode(c.plan, p, g, d, sc, _f32(lr), _f32(decay), 1.0)

        def decode(p, g):
            for c in self.codecs:
                ops.demo_decode(c.plan, c.gathered, p, g, 0.0)
        return place_demo_step(encode, decode, P, G, D)

    def __call__(self, P, G, D, lr, decay=0.999, weight_decay=0.0):
        pending = []
        for c in self.codecs:
            c.encode(P, G, D, lr, decay, weight_decay)
            w = (self.coll.all_gather_into(c.gathered.view(-1), c.payload.view(-1), async_op=True)
                 if self.coll.exchange else DONE)
            pending.append((c, w))
            if len(pending) > 1:
                cp, wp = pending.pop(0)
                wp.wait()
                cp.decode(P, G, lr)
        for cp, wp in pending:
            wp.wait()
            cp.decode(P, G, lr)
