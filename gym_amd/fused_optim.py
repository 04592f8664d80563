"""Inner optimizer on the flat arena.

The reference's strategies run `clip_grad_norm_(model.parameters(), max_norm)`
and `self.optim.step()` with the default inner optimizer torch.optim.AdamW
(exogym/strategy/strategy.py:135-140, diloco.py:52-59,
communicate_optimize_strategy.py:69-74; OptimSpec default optim.py:11).
ArenaAdam is a torch.optim.Optimizer (schedulers such as LambdaLR drive its
param_groups[0]["lr"] as usual) whose step() is ONE fused kernel over the
node's parameter arena (ga_adam_step: read p, g, m, v; write p, m, v) and,
with clipping, one norm reduction (ga_grad_clip_coef) whose coefficient the
step kernel applies on the device -- no host synchronisation.

Exactness: parameters whose .grad is None at step time are skipped, as torch
does: no decay, no moment update, and the parameter's own `step` does not
advance.  torch keeps one `step` per parameter and so does ArenaAdam: while
every parameter has had a gradient on every step they all share one count
tensor (one launch over the whole [K, ld] set, nothing kept per parameter);
when some parameter is absent the parameters fall into groups that share a
count (a group advances with one add, splits when only part of it is present,
and groups that meet on a count merge again), and the kernel runs once per
contiguous arena range whose parameters are present and share a count
(step_size and bc2_sqrt, the bias corrections, are scalars of a launch).  A step on which no parameter has a
gradient launches nothing.  exp_avg / exp_avg_sq of the per-parameter state
are views of the flat state buffers, so state_dict() has torch's layout and
values (a parameter that never had a gradient reports step 0 and zero moments,
where torch has no entry), and load_state_dict() (of an ArenaAdam or a
torch.optim.Adam/AdamW state dict, with equal or different per-parameter
steps) copies the loaded moments into those buffers, so a resumed run
continues where it stopped.

ArenaSGD is the same for OptimSpec(torch.optim.SGD, ...) (the "sgd" of
OptimSpec.from_string, optim.py:24): one ga_sgd_step launch (read p, g, buf;
write p, buf) with momentum, dampening, Nesterov and L2 weight decay, a
per-parameter initialised flag where Adam has a step count.  ArenaMuon is the
"muon" spec (strategy.optim.MuonAdamW): Muon's Newton-Schulz iterations on the
hidden matrices as grouped bf16 MFMA launches over job tables (ga_muon_*), an
inner ArenaAdam on the rest.  ArenaAdafactor is torch.optim.Adafactor (the
"adafactor" spec) on arenas of tensors with at most two dimensions: five launches
over job tables (ga_adafactor_*) that cover all K replicas, and a state of one
row vector and one column vector per matrix instead of full-size moments.
ArenaAdam8bit is the "adamw8bit" spec (strategy.optim.AdamW8bit): AdamW whose two
moments are 8-bit codes under a scale per 64 elements, one ga_adam8_step launch.
build_fused picks the class for a spec; FUSED names them for the callers that
step them.
"""
import math
import time

import torch

from . import ops
from .ops import ADAFACTOR_CHUNK, ADAFACTOR_FIELDS, ADAFACTOR_TILE  # geometry of csrc/adafactor.hip
from .strategy.optim import ADAM8_BLOCK, AdamW8bit, adam_scalars

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")

# physical placement of the moments (gym_amd.placement), chosen on the first step
PLACEMENT_CANDIDATES = 48
PLACEMENT_MAX_FRAC = 0.3
PLACEMENT_MIN_BYTES = 32 << 20
# K > 1 replicas: each replica's moments are placed on their own (probed against that
# replica's parameter / gradient rows), with fewer candidates per replica and a budget:
# a replica's search stops after ROW_PATIENCE candidates unless the best beats its
# ordinary rows by > 2%, and the whole search stops at PLACEMENT_ROW_BUDGET_S
PLACEMENT_ROW_CANDIDATES = 16
PLACEMENT_ROW_PATIENCE = 3
PLACEMENT_ROW_BUDGET_S = 0.25


def _fp32_arena(arena):
    """True for an fp32 arena that has a gradient set (what both fused optimizers step)."""
    grads = getattr(arena, "grad_set", None) if hasattr(arena, "grad_set") else getattr(arena, "grad_flat", None)
    return arena is not None and grads is not None and arena.dtype == torch.float32


def fusable(spec_cls, kwargs, arena):
    """True when OptimSpec(spec_cls, **kwargs) can run as ArenaAdam on this arena."""
    if spec_cls not in (torch.optim.AdamW, torch.optim.Adam) or not _fp32_arena(arena):
        return False
    kw = dict(kwargs or {})
    if any(kw.get(k) for k in _UNSUPPORTED):
        return False
    if spec_cls is torch.optim.Adam and kw.get("decoupled_weight_decay"):
        return False
    allowed = {"lr", "betas", "eps", "weight_decay", "foreach", "fused"} | set(_UNSUPPORTED)
    if set(kw) - allowed:
        return False
    lr = kw.get("lr", 1e-3)
    return not isinstance(lr, torch.Tensor)


def place_moment_rows(P, G, Mr, Vr, max_candidates=None, max_frac=None, patience=None, budget_s=None):
    """Per-replica placement of Adam moments (ArenaAdam, K > 1): for each
    replica k, fresh allocations of its two moment rows are timed with
    ga_probe_adam_placement against P[k], G[k] (values unchanged) beside Mr[k],
    Vr[k] where they are; the fastest keeps them.  Budget: up to max_candidates
    per replica, stopping after `patience` unless the best beats the rows' own
    time by > 2% (placement.choose), and the whole search ends by budget_s (each
    replica gets an equal share of what is left).  Rows not moved stay where
    they were probed (views of the caller's buffers).  Returns (new rows M, new
    rows V, per replica the chosen buffer or None, the record)."""
    from . import placement
    max_candidates = PLACEMENT_ROW_CANDIDATES if max_candidates is None else max_candidates
    max_frac = PLACEMENT_MAX_FRAC if max_frac is None else max_frac
    patience = PLACEMENT_ROW_PATIENCE if patience is None else patience
    budget_s = PLACEMENT_ROW_BUDGET_S if budget_s is None else budget_s
    watch = placement.Stopwatch()
    t_end = watch.t0 + budget_s
    K, ld = P.shape[0], Mr[0].numel()
    bufs, probe_ms, chosen = [], [], []
    for k in range(K):
        Pk, Gk = P[k, :ld], G[k, :ld]

        def probe(M, V):
            return placement.time_probe(lambda: ops.probe_adam_placement(Pk, Gk, M, V), reps=2)

        def split(buf):
            t = buf.tensor()
            return t[:ld], t[ld:2 * ld]

        now = time.perf_counter()
        deadline = now + max(0.0, t_end - now) / (K - k)
        best, times = placement.choose(2 * ld * 4, P.device, lambda b: probe(*split(b)), probe(Mr[k], Vr[k]),
                                       max_candidates, max_frac, patience=patience, deadline=deadline)
        bufs.append(best)
        probe_ms.append([round(t, 4) for t in times])
        chosen.append(min(range(len(times)), key=lambda i: times[i]) if best is not None else 0)
    outM, outV = [], []
    for k, b in enumerate(bufs):
        if b is None:  # kept where they were probed
            m, v = Mr[k], Vr[k]
        else:
            t = b.tensor()
            m, v = t[:ld], t[ld:2 * ld]
            m.copy_(Mr[k])
            v.copy_(Vr[k])
        outM.append(m)
        outV.append(v)
    rec = {"per_replica": True, "candidates_per_replica": max_candidates, "patience": patience,
           "budget_s": budget_s, "candidates_probed": sum(len(t) - 1 for t in probe_ms), "chosen": chosen,
           "placed_rows": sum(b is not None for b in bufs),
           "probe_ms_ordinary_sum": round(sum(t[0] for t in probe_ms), 4),
           "probe_ms_chosen_sum": round(sum(min(t) for t in probe_ms), 4), "probe_ms": probe_ms}
    return outM, outV, bufs, watch.stamp(rec)


class _ArenaOptimizer(torch.optim.Optimizer):
    """What ArenaAdam and ArenaSGD share: the binding to one node's ParamArena or
    a ReplicaArena, the clip buffers, the joining of present parameters into
    launch ranges, and step().  A subclass supplies _ranges (the present
    parameters under their key: what a launch's scalars depend on), _prepare
    (what must be in place before launching), _launch and, where a step leaves
    something per parameter, _finish."""

    def __init__(self, params, defaults, arena):
        super().__init__(params, defaults)
        name = type(self).__name__
        if len(self.param_groups) != 1:
            raise ValueError(f"{name}: one parameter group (the node's arena)")
        self.arenas = list(getattr(arena, "arenas", [arena]))
        self._arena = arena  # P and G are read from it at every use: the sets may be relocated
        self.K, self.ld = self.P.shape
        where = {}
        for k, ar in enumerate(self.arenas):
            for i, p in enumerate(ar.params):
                where[id(p)] = (k, ar.layout.offsets[i], ar.layout.numels[i])
        self._where = where
        self._spans = [[] for _ in self.arenas]  # per replica: (param, offset, numel) in arena order
        for p in self.param_groups[0]["params"]:
            if id(p) not in where:
                raise ValueError(f"{name}: every parameter must live in the arena")
            k, o, n = where[id(p)]
            self._spans[k].append((p, o, n))
        for sp in self._spans:
            sp.sort(key=lambda t: t[1])
        # an optimizer that owns only part of the arena (ArenaMuon's inner ArenaAdam) never
        # steps a whole row: the other tensors belong to someone else
        self._owns_arena = all(len(sp) == len(ar.params) for sp, ar in zip(self._spans, self.arenas))
        self._partials = ops.sumsq_partials(self.P.device, self.K)
        self._clip = torch.ones(2 * self.K, dtype=torch.float32, device=self.P.device)

    @property
    def P(self):
        """The parameter set [K, ld] (the replica arena's rows, or the node's arena as one row)."""
        a = self._arena
        return a.flat_set if hasattr(a, "flat_set") else a.flat.view(1, -1)

    @property
    def G(self):
        """The gradient set, read from the arena like P."""
        a = self._arena
        return a.grad_set if hasattr(a, "grad_set") else a.grad_flat.view(1, -1)

    def _join(self, live):
        """live: per replica the (offset, numel, key) spans of its present
        parameters, sorted.  Returns per replica [(a, b, key)]: the contiguous
        ranges of present parameters that share the key -- adjacent spans (only
        zero padding, < 64 elements, between them) joined, and the whole row
        when all of a replica are present on one key: the padding stays 0."""
        ranges = []
        for k, spans in enumerate(live):
            out = []
            for o, n, key in spans:
                if out and o - out[-1][1] < 64 and out[-1][2] == key:
                    out[-1][1] = o + n
                else:
                    out.append([o, o + n, key])
            if len(out) == 1 and len(spans) == len(self._spans[k]) and self._owns_arena:
                out = [[0, self.ld, out[0][2]]]
            ranges.append([tuple(r) for r in out])
        return ranges

    _whole_set = True  # one launch may cover the [K, ld] sets when every replica has the same whole-row range

    def _finish(self):
        pass

    @torch.no_grad()
    def step(self, closure=None, max_norm=None, clip=None):
        """clip: the coefficients of a ga_grad_clip_coef the caller already ran over
        the gradient set (ArenaMuon clips both of its parts by one norm)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ranges = self._ranges()
        for ar in self.arenas:
            ar.sync_grads()
        if not any(ranges):  # no parameter has a gradient: torch's step does nothing
            return loss
        self._prepare()
        if clip is None and max_norm:
            ops.grad_clip_coef(self.G, self.ld, max_norm, self._partials, self._clip)
            clip = self._clip
        whole = ranges[0]
        if self._whole_set and whole and whole[0][:2] == (0, self.ld) and all(r == whole for r in ranges):
            self._launch(None, 0, self.ld, whole[0][2], clip)
        else:
            for k in range(self.K):  # per replica: partial ranges, keys apart, or state rows placed apart
                ck = clip[2 * k:2 * k + 2] if clip is not None else None
                for a, b, key in ranges[k]:
                    self._launch(k, a, b, key, ck)
        self._finish()
        return loss


class _AdamCounts:
    """What ArenaAdam and ArenaAdam8bit share beside _ArenaOptimizer: a step count per
    parameter kept as groups of parameters that share one count tensor, the launch
    ranges of the present parameters by count, and the launch scalars.  The class
    supplies _bind_state(p): state[p] with its `step` kept and its moments re-pointed."""

    def _start_counts(self):
        # the step counts: [count tensor, [(param, replica, offset, numel)]] per group of parameters that
        # share a count -- state[p]["step"] of its members IS the group's tensor, so a step advances a
        # group with one add.  One group while every parameter has had a gradient on every step.
        self._groups = [[torch.tensor(0.0), []]]
        for p in self.param_groups[0]["params"]:
            self._groups[0][1].append((p, *self._where[id(p)]))
            self._bind_state(p)

    def state_dict(self):
        """torch's layout, every parameter with a `step` tensor of its own (here
        the parameters of a group share one; torch's optimizers, which advance
        each entry in place, must not)."""
        sd = super().state_dict()
        sd["state"] = {i: {**st, "step": st["step"].clone()} for i, st in sd["state"].items()}
        return sd

    def _regroup(self, steps):
        """steps: id(param) -> its loaded count.  One group, and one count tensor, per distinct count."""
        groups = {}
        for k, sp in enumerate(self._spans):
            for p, o, n in sp:
                t = steps[id(p)]
                g = groups.get(t) or groups.setdefault(t, [torch.tensor(t), []])
                g[1].append((p, k, o, n))
                self.state[p]["step"] = g[0]
                self._bind_state(p)
        self._groups = list(groups.values())

    def _ranges(self):
        """Advance the count of every parameter that has a gradient now and
        return, per replica, [(a, b, t)]: the contiguous ranges of present
        parameters that share the count t (_join).  A group whose members
        are all present advances with one add; one that is partly present
        splits; groups that reach the same count become one again."""
        groups = self._groups
        if self._owns_arena and len(groups) == 1 and all(m[0].grad is not None for m in groups[0][1]):
            groups[0][0] += 1  # every parameter present on one count: nothing per parameter
            return [[(0, self.ld, float(groups[0][0]))]] * self.K
        live = [[] for _ in range(self.K)]
        merged = {}  # count -> [its tensor, members]
        for clock, members in groups:
            here = [m for m in members if m[0].grad is not None]
            if len(here) == len(members):
                clock += 1
                parts = [(clock, members)]
            elif not here:
                parts = [(clock, members)]
            else:  # the present members go on with a count tensor of their own
                parts = [(clock, [m for m in members if m[0].grad is None]), (clock + 1, here)]
            if here:
                t = float(parts[-1][0])
                for _, k, o, n in here:
                    live[k].append((o, n, t))
            for c, ms in parts:
                into = merged.setdefault(float(c), [c, []])
                into[1].extend(ms)
                if into[0] is not clock:
                    for m in ms:
                        self.state[m[0]]["step"] = into[0]
        self._groups = list(merged.values())
        return self._join([sorted(spans) for spans in live])

    def _hp(self, t):
        """The launch scalars of a step at count t (torch's _single_tensor_adam)."""
        return adam_scalars(self.param_groups[0], t)


class ArenaAdam(_AdamCounts, _ArenaOptimizer):
    """Adam/AdamW over one node's ParamArena, or over a ReplicaArena (K nodes of
    one process, [K, ld] parameter/gradient sets: one launch for all of them,
    each replica clipped by its own gradient norm)."""

    def __init__(self, params, arena, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None, decoupled=True,
                 placement=True, **ignored):
        if weight_decay is None:
            weight_decay = 1e-2 if decoupled else 0.0  # torch's AdamW / Adam defaults
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        for i, b in enumerate(betas):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"Invalid beta parameter at index {i}: {b}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                        maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=bool(decoupled))
        super().__init__(params, defaults, arena)
        self._M = torch.zeros_like(self.P, dtype=torch.float32)
        self._V = torch.zeros_like(self.P, dtype=torch.float32)
        # per replica [ld] rows of the moments: views of _M / _V, or (after a per-replica
        # placement) each in its own candidate buffer, when _M / _V are None
        self._Mr, self._Vr = list(self._M.unbind(0)), list(self._V.unbind(0))
        self.exp_avg, self.exp_avg_sq = self._M.view(-1), self._V.view(-1)  # flat views (single-arena users)
        self._start_counts()
        self._placed = None  # the candidate buffer holding M and V once _place chose one
        self._placed_for = None  # (P, G) data pointers the moments were placed against
        self._placements = 0  # searches run (a relocated P / G set is searched again)
        self.placement = None  # the placement record (probe times, or why it was skipped)
        self.place_opt = placement  # False: never probe / move the moments (gym_amd.placement.policy)

    @property
    def M(self):
        """exp_avg as [K, ld] (a stacked copy once the rows were placed apart)."""
        return self._M if self._M is not None else torch.stack(self._Mr)

    @property
    def V(self):
        return self._V if self._V is not None else torch.stack(self._Vr)

    def _bind_state(self, p):
        k, o, n = self._where[id(p)]
        st = self.state.get(p)
        step = st["step"] if st else self._groups[0][0]  # its group's count tensor
        self.state[p] = {"step": step, "exp_avg": self._Mr[k][o:o + n].view(p.shape),
                         "exp_avg_sq": self._Vr[k][o:o + n].view(p.shape)}

    def load_state_dict(self, state_dict):
        """torch's Optimizer.load_state_dict, then the loaded per-parameter
        moments are copied into the flat state buffers the kernel reads and the
        state is re-pointed at those views.  Parameters may carry different
        `step` counts (torch's do once one of them missed a gradient); one
        without an entry starts at step 0 with zero moments."""
        super().load_state_dict(state_dict)
        steps = {}
        with torch.no_grad():
            for r in self._Mr + self._Vr:
                r.zero_()
            for p in self.param_groups[0]["params"]:
                st = self.state.get(p, {})
                k, o, n = self._where[id(p)]
                if "exp_avg" in st:
                    self._Mr[k][o:o + n].copy_(st["exp_avg"].reshape(-1))
                    self._Vr[k][o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
                steps[id(p)] = float(st["step"]) if "step" in st else 0.0
        self._regroup(steps)

    def _place(self):
        """Choose the physical memory of the moments, once, before the first
        step: the fused step's rate depends on where exp_avg / exp_avg_sq sit
        physically relative to the parameters and gradients (0.553-0.625 ms at
        GPT-2 124M, profiles/r04k_adam_placement.txt; gym_amd.placement), so
        fresh device allocations are timed with ga_probe_adam_placement (the
        step's access pattern, values unchanged) beside the ordinary ones and
        the fastest keeps the moments.  One replica (K = 1): up to
        PLACEMENT_CANDIDATES buffers for both moments.  K > 1: replica by
        replica, up to PLACEMENT_ROW_CANDIDATES buffers of one replica's two
        moment rows each, probed against that replica's parameter / gradient
        rows (the kernel's replica-major grid streams one replica's four rows
        at a time; a [K, ld] candidate at K = 32 x 124M would be 32 GB, so the
        memory budget would leave no choice); the step then runs one launch
        per replica.  When the parameter / gradient set is later moved (the
        outer step's own placement relocates the replica set at step H), the
        search runs again against the new rows, so the moments' placement
        always describes the step that runs."""
        self._placed_for = (self.P.data_ptr(), self.G.data_ptr())
        self._placements += 1
        nb = 2 * self.K * self.ld * 4
        if (self.P.device.type != "cuda" or nb < PLACEMENT_MIN_BYTES or PLACEMENT_CANDIDATES < 2
                or self.ld % 4 or self.P.stride(-1) != 1):
            return
        from . import placement
        ok, why = placement.policy(self.place_opt)
        if not ok:
            self.placement = {"placed": False, "why": why}
            return
        watch = placement.Stopwatch()
        if self.K == 1:
            self._place_whole(placement, nb)
        else:
            self._place_rows(placement)
        watch.stamp(self.placement)
        self.placement["searches"] = self._placements

    def _place_whole(self, placement, nb):
        KL = self.K * self.ld

        def probe(M, V):
            return placement.time_probe(lambda: ops.probe_adam_placement(self.P, self.G, M, V))

        def split(buf):
            t = buf.tensor()
            return t[:KL].view(self.K, self.ld), t[KL:2 * KL].view(self.K, self.ld)

        best, times = placement.choose(nb, self.P.device, lambda b: probe(*split(b)), probe(self._M, self._V),
                                       PLACEMENT_CANDIDATES, PLACEMENT_MAX_FRAC)
        chosen = 0
        if best is not None:
            chosen = min(range(len(times)), key=lambda i: times[i])
            self.move_moments(*split(best), owner=best)
        self.placement = {"candidates": len(times), "probe_ms": [round(t, 4) for t in times], "chosen": chosen}

    def move_moments(self, M, V, owner=None):
        """Move exp_avg / exp_avg_sq into other [K, ld] fp32 buffers (contents
        copied, the per-parameter state re-pointed); `owner` keeps their memory
        alive.  The placement search's move, also open to a caller that wants
        the moments in memory of its own."""
        if M.shape != self.P.shape or V.shape != self.P.shape or M.dtype != torch.float32 or V.dtype != torch.float32:
            raise ValueError("ArenaAdam.move_moments: [K, ld] float32 buffers")
        with torch.no_grad():
            M.copy_(self.M)
            V.copy_(self.V)
        self._M, self._V, self._placed = M, V, owner
        self._Mr, self._Vr = list(M.unbind(0)), list(V.unbind(0))
        self.exp_avg, self.exp_avg_sq = M.view(-1), V.view(-1)
        for p in self.param_groups[0]["params"]:
            self._bind_state(p)

    def _place_rows(self, placement):
        Mr, Vr, bufs, rec = place_moment_rows(self.P, self.G, self._Mr, self._Vr)
        if any(b is not None for b in bufs):
            self._Mr, self._Vr, self._placed = Mr, Vr, bufs
            self._M = self._V = None
            self.exp_avg = self.exp_avg_sq = None
            for p in self.param_groups[0]["params"]:
                self._bind_state(p)
            torch.cuda.empty_cache()
        self.placement = rec

    @property
    def _whole_set(self):
        return self._M is not None  # rows placed apart take one launch each

    def _prepare(self):
        if self._placed_for != (self.P.data_ptr(), self.G.data_ptr()):
            self._place()
        self._hps = {}  # the launch scalars per count of this step

    def _launch(self, k, a, b, t, clip):
        hp = self._hps.get(t) or self._hps.setdefault(t, self._hp(t))
        if k is None:
            ops.adam_step(self.P, self.G, self._M, self._V, clip_coef=clip, **hp)
        else:
            ops.adam_step(self.P[k, a:b], self.G[k, a:b], self._Mr[k][a:b], self._Vr[k][a:b], clip_coef=clip, **hp)


def fusable_adam8(spec_cls, kwargs, arena):
    """True when OptimSpec(spec_cls, **kwargs) can run as ArenaAdam8bit on this arena:
    AdamW8bit on an fp32 arena with a gradient set, a float learning rate."""
    if spec_cls is not AdamW8bit or not _fp32_arena(arena):
        return False
    kw = dict(kwargs or {})
    return not set(kw) - set(_ADAM8_KW) and not isinstance(kw.get("lr", 1e-3), torch.Tensor)


_ADAM8_KW = ("lr", "betas", "eps", "weight_decay")


class ArenaAdam8bit(_AdamCounts, _ArenaOptimizer):
    """AdamW8bit (gym_amd.strategy.optim: AdamW with block-wise 8-bit moments) over one
    node's ParamArena or a ReplicaArena: step() is one ga_adam8_step launch over the
    [K, ld] sets and, with clipping, one ga_grad_clip_coef.  Counts, absent parameters
    and launch ranges as ArenaAdam's (_AdamCounts); not an ArenaAdam, so nothing that
    reaches for fp32 moments mistakes it for one.

    The moments are two uint8 [K, ld] code sets and two fp32 [K, ld / 64] scale sets: 2.125
    bytes per arena element and replica where ArenaAdam has 8.  Arena tensors start at
    multiples of 64 elements and the padding between them is zero, so a block never holds
    two tensors and a launch range, its end rounded up to a block, only takes the last
    tensor's own padding along, which stays zero under the update.  state[p] holds
    `step` and, as views of the flat sets, AdamW8bit's exp_avg_code / exp_avg_absmax /
    exp_avg_sq_code / exp_avg_sq_absmax over the tensor's whole blocks, so state_dict() has
    AdamW8bit's layout; load_state_dict() takes either class's dict, or a
    torch.optim.AdamW / Adam / ArenaAdam dict, whose fp32 moments are quantised by
    ga_adam8_encode."""

    def __init__(self, params, arena, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, placement=True):
        defaults = AdamW8bit([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults
        super().__init__(params, defaults, arena)
        if self.ld % ADAM8_BLOCK or any(o % ADAM8_BLOCK for sp in self._spans for _, o, _ in sp):
            raise ValueError("ArenaAdam8bit: arena tensors must start at multiples of 64 elements")
        dev, nb = self.P.device, self.ld // ADAM8_BLOCK
        self._Mc = torch.full((self.K, self.ld), 127, dtype=torch.uint8, device=dev)  # the signed row's zero
        self._Vc = torch.zeros(self.K, self.ld, dtype=torch.uint8, device=dev)
        self._Ma = torch.zeros(self.K, nb, dtype=torch.float32, device=dev)
        self._Va = torch.zeros(self.K, nb, dtype=torch.float32, device=dev)
        self._start_counts()
        self.placement = {"placed": False, "why": "no search for 8-bit AdamW"}

    def state_bytes(self):
        return sum(t.numel() * t.element_size() for t in (self._Mc, self._Vc, self._Ma, self._Va))

    def _bind_state(self, p):
        k, o, n = self._where[id(p)]
        st = self.state.get(p)
        a, b = o // ADAM8_BLOCK, (o + n + ADAM8_BLOCK - 1) // ADAM8_BLOCK  # the tensor's whole blocks
        self.state[p] = {"step": st["step"] if st else self._groups[0][0],
                         "exp_avg_code": self._Mc[k, a * ADAM8_BLOCK:b * ADAM8_BLOCK], "exp_avg_absmax": self._Ma[k, a:b],
                         "exp_avg_sq_code": self._Vc[k, a * ADAM8_BLOCK:b * ADAM8_BLOCK],
                         "exp_avg_sq_absmax": self._Va[k, a:b]}

    def load_state_dict(self, state_dict):
        """torch's Optimizer.load_state_dict, then the loaded moments go into the flat
        sets and the state is re-pointed at their views: codes and scales are copied,
        fp32 exp_avg / exp_avg_sq (a torch.optim.AdamW or ArenaAdam dict) are quantised
        row by row with ga_adam8_encode.  A parameter without an entry starts at step 0
        with zero moments."""
        super().load_state_dict(state_dict)
        loaded = {id(p): dict(self.state.get(p, {})) for p in self.param_groups[0]["params"]}
        with torch.no_grad():
            self._Mc.fill_(127)
            for t in (self._Vc, self._Ma, self._Va):
                t.zero_()
            for k, sp in enumerate(self._spans):
                full = [(o, n, loaded[id(p)]) for p, o, n in sp if "exp_avg" in loaded[id(p)]]
                if full:  # encode the row's fp32 moments, then keep only these tensors' blocks
                    rows = torch.zeros(2, self.ld, dtype=torch.float32, device=self.P.device)
                    for o, n, st in full:
                        rows[0, o:o + n].copy_(st["exp_avg"].reshape(-1))
                        rows[1, o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
                    ops.adam8_encode(rows[0], self._Mc[k], self._Ma[k], 0)
                    ops.adam8_encode(rows[1], self._Vc[k], self._Va[k], 1)
                for p, o, n in sp:
                    st = loaded[id(p)]
                    self.state[p] = {"step": None}
                    self._bind_state(p)
                    for key in ("exp_avg_code", "exp_avg_absmax", "exp_avg_sq_code", "exp_avg_sq_absmax"):
                        if key in st:
                            self.state[p][key].copy_(st[key].reshape(-1))
        self._regroup({i: float(st["step"]) if "step" in st else 0.0 for i, st in loaded.items()})

    def _prepare(self):
        self._hps = {}  # the launch scalars per count of this step

    def _launch(self, k, a, b, t, clip):
        hp = self._hps.get(t) or self._hps.setdefault(t, self._hp(t))
        if k is None:
            ops.adam8_step(self.P, self.G, self._Mc, self._Ma, self._Vc, self._Va, clip_coef=clip, **hp)
            return
        b = (b + ADAM8_BLOCK - 1) // ADAM8_BLOCK * ADAM8_BLOCK  # the last tensor's own zero padding
        ba, bb = a // ADAM8_BLOCK, b // ADAM8_BLOCK
        ops.adam8_step(self.P[k, a:b], self.G[k, a:b], self._Mc[k, a:b], self._Ma[k, ba:bb], self._Vc[k, a:b],
                       self._Va[k, ba:bb], clip_coef=clip, **hp)


_SGD_KW = ("lr", "momentum", "dampening", "weight_decay", "nesterov")


def fusable_sgd(spec_cls, kwargs, arena):
    """True when OptimSpec(spec_cls, **kwargs) can run as ArenaSGD on this arena:
    torch.optim.SGD on an fp32 arena with a gradient set, no maximize /
    differentiable, a float learning rate."""
    if spec_cls is not torch.optim.SGD or not _fp32_arena(arena):
        return False
    kw = dict(kwargs or {})
    if kw.get("maximize") or kw.get("differentiable"):
        return False
    if set(kw) - (set(_SGD_KW) | {"foreach", "fused", "maximize", "differentiable"}):
        return False
    return not isinstance(kw.get("lr", 1e-3), torch.Tensor)


class ArenaSGD(_ArenaOptimizer):
    """torch.optim.SGD (momentum, dampening, Nesterov, L2 weight decay) over one
    node's ParamArena or a ReplicaArena, built as ArenaAdam is: step() is one
    ga_sgd_step launch over the [K, ld] sets (read p, g, buf; write p, buf) and,
    with clipping, one ga_grad_clip_coef whose coefficient the step applies on
    the device.

    Exactness, as torch's: a parameter whose .grad is None at step time keeps its
    value and its buffer; torch creates a parameter's momentum buffer as a clone
    of the first gradient it ever sees (no dampening on that step), so every
    parameter carries an *initialised* flag and a parameter that joins late takes
    its own `first` launch while its neighbours take the ordinary one.  While
    every parameter is present on one flag the step is one launch; otherwise the
    kernel runs once per contiguous arena range of present parameters that share
    the flag.  The buffer is one fp32 [K, ld] set (none while momentum is 0);
    state[p]["momentum_buffer"] is a view of it once p has had a gradient and
    None before (torch has no entry then), so state_dict() has torch's layout and
    load_state_dict() takes an ArenaSGD or a torch.optim.SGD state dict."""

    def __init__(self, params, arena, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False,
                 placement=True, **ignored):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, arena)
        self._B = None  # the momentum buffer [K, ld], allocated when momentum != 0
        self._owner = None  # keeps a caller's buffer memory alive (move_buffer)
        self._inited = set()  # ids of the parameters whose buffer holds their first gradient
        if momentum != 0:
            self._buffer()
        self.placement = {"placed": False, "why": "no search for SGD"}

    @property
    def B(self):
        """The momentum buffer [K, ld] (None while momentum has been 0)."""
        return self._B

    def _buffer(self):
        if self._B is None:
            self._B = torch.zeros_like(self.P, dtype=torch.float32)
            for p in self.param_groups[0]["params"]:
                self._bind_state(p)
        return self._B

    def _bind_state(self, p):
        k, o, n = self._where[id(p)]
        self.state[p] = {"momentum_buffer": self._B[k, o:o + n].view(p.shape) if id(p) in self._inited else None}

    def move_buffer(self, B, owner=None):
        """Move the momentum buffer into another [K, ld] fp32 buffer (contents
        copied, the per-parameter state re-pointed); `owner` keeps its memory
        alive.  The counterpart of ArenaAdam.move_moments, for a caller that
        wants the buffer in memory of its own."""
        if B.shape != self.P.shape or B.dtype != torch.float32:
            raise ValueError("ArenaSGD.move_buffer: a [K, ld] float32 buffer")
        with torch.no_grad():
            if self._B is not None:
                B.copy_(self._B)
            else:
                B.zero_()
        self._B, self._owner = B, owner
        for p in self.param_groups[0]["params"]:
            self._bind_state(p)

    def load_state_dict(self, state_dict):
        """torch's Optimizer.load_state_dict, then the loaded per-parameter
        buffers are copied into the flat buffer the kernel reads and the state is
        re-pointed at those views.  `momentum_buffer: None` or no entry: the
        parameter is not initialised (its next gradient is its first)."""
        super().load_state_dict(state_dict)
        loaded = {id(p): self.state.get(p, {}).get("momentum_buffer") for p in self.param_groups[0]["params"]}
        self._inited = {i for i, b in loaded.items() if b is not None}
        if not self._inited and self._B is None and self.param_groups[0]["momentum"] == 0:
            self.state.clear()
            return
        if self._B is None:
            self._B = torch.zeros_like(self.P, dtype=torch.float32)
        with torch.no_grad():
            self._B.zero_()
            for p in self.param_groups[0]["params"]:
                if loaded[id(p)] is not None:
                    k, o, n = self._where[id(p)]
                    self._B[k, o:o + n].copy_(loaded[id(p)].reshape(-1))
                self._bind_state(p)

    def _ranges(self):
        """Per replica [(a, b, first)]: the contiguous ranges of present parameters
        that share the flag (_join); self._fresh lists the present parameters
        that are not initialised yet.  Without momentum there is no buffer and no
        flag (torch creates none)."""
        with_momentum = float(self.param_groups[0]["momentum"]) != 0
        live, self._fresh = [], []
        for spans in self._spans:
            live.append([])
            for p, o, n in spans:
                if p.grad is None:
                    continue
                first = with_momentum and id(p) not in self._inited
                if first:
                    self._fresh.append(p)
                live[-1].append((o, n, first))
        return self._join(live)

    def _prepare(self):
        g = self.param_groups[0]
        # neg_lr and 1 - dampening in double, rounded once (torch's alpha=-lr, alpha=1 - dampening)
        self._hp = dict(neg_lr=-float(g["lr"]), momentum=float(g["momentum"]),
                        one_m_dampening=1 - float(g["dampening"]), weight_decay=float(g["weight_decay"]),
                        nesterov=bool(g["nesterov"]))
        if self._hp["momentum"] != 0:
            self._buffer()

    def _launch(self, k, a, b, first, clip):
        B = self._B if self._hp["momentum"] != 0 else None
        if k is None:
            ops.sgd_step(self.P, self.G, B, first=first, clip_coef=clip, **self._hp)
        else:
            ops.sgd_step(self.P[k, a:b], self.G[k, a:b], B[k, a:b] if B is not None else None, first=first,
                         clip_coef=clip, **self._hp)

    def _finish(self):
        for p in self._fresh:  # their buffers now hold their first gradient
            self._inited.add(id(p))
            self._bind_state(p)


# the "muon" spec without a `fused` kwarg: ArenaMuon, which was 3.5-4.1x faster than the unfused
# MuonAdamW in every alternated pair at K = 1 and K = 8 (profiles/inner_muon.txt); fused=False opts out
MUON_FUSED_DEFAULT = True
MUON_PLAN_CACHE = 8  # present sets whose device tables an ArenaMuon keeps (least recently used evicted)


def _round_up(x, m):
    return (x + m - 1) // m * m


class MuonPlan:
    """The device tables of one Muon pass over a replica row (include/gym_amd.h,
    "Muon inner step"), for the matrices `present` of `slots`: the matrix table,
    the prepare / apply jobs (64 x 64 tiles of each parameter), and per macro-tile
    class (128, or 64 for matrices whose short side fits one 64 tile) the jobs of
    the symmetric products (tile column >= tile row) and of the update (every
    tile).  slots: per Muon matrix (offset, rows, cols, tile, m_pad, n_pad, x,
    xt0, xt1, a, b, ratio), the workspace offsets fixed for the arena layout
    whichever matrices are present, so a matrix's padding only ever receives the
    zeros its own products compute."""

    def __init__(self, slots, present, device):
        import struct
        F = ops.muon_fields()
        P = ops.MUON_PREP_TILE
        mats, prep = [], []
        sym, upd = {64: [], 128: []}, {64: [], 128: []}
        for t, s in enumerate(slots[i] for i in present):
            off, rows, cols, tile, m_pad, n_pad, x, xt0, xt1, a, b, ratio = s
            job0 = len(prep)
            prep += [(t, i, j, 0) for i in range(-(-rows // P)) for j in range(-(-cols // P))]
            bits = struct.unpack("<I", struct.pack("<f", ratio))[0]
            row = [off, rows, cols, m_pad, n_pad, x, xt0, xt1, a, b, int(rows > cols), job0, len(prep) - job0, bits]
            mats.append(row + [0] * (F - len(row)))
            mt, nt = m_pad // tile, n_pad // tile
            sym[tile] += [(t, i, j, 0) for i in range(mt) for j in range(i, mt)]
            upd[tile] += [(t, i, j, 0) for i in range(mt) for j in range(nt)]

        def table(rows, dtype, width):
            return torch.tensor(rows, dtype=dtype).reshape(-1, width).to(device)

        self.nmats = len(mats)
        self.mats = table(mats, torch.int64, F)
        self.prep = table(prep, torch.int32, 4)
        self.classes = [(T, table(sym[T], torch.int32, 4), table(upd[T], torch.int32, 4)) for T in (128, 64) if sym[T]]
        self.partials = torch.zeros(max(len(prep), 1), dtype=torch.float32, device=device)
        self.scale = torch.ones(max(len(mats), 1), dtype=torch.float32, device=device)


class ArenaMuon(torch.optim.Optimizer):
    """MuonAdamW (gym_amd.strategy.optim) over one node's ParamArena or a
    ReplicaArena: torch.optim.Muon on the Muon matrices as grouped launches over
    job tables (ga_muon_prepare, ga_muon_scale, 3 x ns_steps ga_muon_gemm,
    ga_muon_apply: ~18 launches per replica where torch issues 15 GEMMs and as
    many elementwise ops per matrix), and an inner ArenaAdam (AdamW) on every
    other parameter.  param_groups[0] is Muon's group and param_groups[1] the
    inner ArenaAdam's own, so a scheduler drives both learning rates.

    muon_mask: a bool per parameter of one replica, in arena order
    (strategy.optim.muon_matrix_mask).  The momentum is one fp32 [K, ld] set (4
    bytes per arena element and replica, beside the inner ArenaAdam's two [K, ld]
    moment sets: 12 bytes per arena element and replica in all); state[p]["momentum_buffer"] are views of
    it, torch's state_dict layout.  The bf16 workspace (X, two copies of X^T, A and
    B per matrix, padded to whole tiles) holds ONE replica's matrices: the K
    replicas take their passes in turn.  step(max_norm=) clips both parts by one
    coefficient per replica over its whole gradient row.  A matrix whose .grad is
    None is skipped exactly (no decay, no buffer change): the job tables are built
    for the present set and cached by it.  No host synchronisation in a step."""

    def __init__(self, params, arena, muon_mask, lr=1e-3, weight_decay=0.1, momentum=0.95, nesterov=True,
                 ns_coefficients=(3.4445, -4.775, 2.0315), eps=1e-7, ns_steps=5, adjust_lr_fn=None, adamw_lr=1e-3,
                 adamw_betas=(0.9, 0.999), adamw_eps=1e-8, adamw_weight_decay=1e-2, placement=True):
        if lr < 0.0 or adamw_lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}, {adamw_lr}")
        if not 0.0 <= momentum < 1.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if len(ns_coefficients) != 3 or not 0 <= int(ns_steps) < 100:
            raise ValueError("ArenaMuon: three ns_coefficients and 0 <= ns_steps < 100")
        arenas = list(getattr(arena, "arenas", [arena]))
        muon_mask = [bool(m) for m in muon_mask]
        if any(len(ar.params) != len(muon_mask) for ar in arenas):
            raise ValueError("ArenaMuon: muon_mask must hold a bool per parameter of a replica")
        given = {id(p) for p in params}
        mats = [[p for p, m in zip(ar.params, muon_mask) if m] for ar in arenas]
        rest = [p for ar in arenas for p, m in zip(ar.params, muon_mask) if not m and p.requires_grad]
        if not all(id(p) in given for ps in mats for p in ps) or not all(id(p) in given for p in rest):
            raise ValueError("ArenaMuon: every parameter must live in the arena")
        if not mats[0]:
            raise ValueError("ArenaMuon: no Muon matrix selected")
        self.adam = ArenaAdam(rest, arena, lr=adamw_lr, betas=adamw_betas, eps=adamw_eps,
                              weight_decay=adamw_weight_decay, decoupled=True, placement=placement) if rest else None
        group = dict(params=[p for ps in mats for p in ps], lr=lr, weight_decay=weight_decay, momentum=momentum,
                     nesterov=bool(nesterov), ns_coefficients=tuple(ns_coefficients), eps=eps, ns_steps=int(ns_steps),
                     adjust_lr_fn=adjust_lr_fn)
        super().__init__([group] + ([self.adam.param_groups[0]] if self.adam else []), {})
        self.arenas, self._arena = arenas, arena
        self.K, self.ld = self.P.shape
        self.muon_mask = muon_mask
        self._mats = mats
        layout = arenas[0].layout
        self._slots, ws = [], 0
        for i, m in enumerate(muon_mask):
            if not m:
                continue
            shape = layout.shapes[i]
            if len(shape) != 2:
                raise ValueError(f"ArenaMuon: a Muon parameter must be 2-D, got {shape}")
            rows, cols = shape
            tile = 64 if min(rows, cols) <= 64 else 128
            m_pad, n_pad = _round_up(min(rows, cols), tile), _round_up(max(rows, cols), tile)
            x, xt0, xt1 = ws, ws + m_pad * n_pad, ws + 2 * m_pad * n_pad
            a, b = ws + 3 * m_pad * n_pad, ws + 3 * m_pad * n_pad + m_pad * m_pad
            ws += 3 * m_pad * n_pad + 2 * m_pad * m_pad
            self._slots.append((layout.offsets[i], rows, cols, tile, m_pad, n_pad, x, xt0, xt1, a, b,
                                self._ratio(adjust_lr_fn, rows, cols)))
        dev = self.P.device
        self.workspace = torch.zeros(ws, dtype=torch.bfloat16, device=dev)
        self._B = torch.zeros_like(self.P, dtype=torch.float32)
        self._plans = {}  # present matrices (indices into _slots) -> MuonPlan
        self._partials = ops.sumsq_partials(dev, self.K)
        self._clip = torch.ones(2 * self.K, dtype=torch.float32, device=dev)
        if self.adam is not None:  # one state dict: torch's per-parameter entries of both parts
            self.state.update(self.adam.state)
            self.adam.state = self.state
        self._bind_state()
        self.placement = self.adam.placement if self.adam else None

    @staticmethod
    def _ratio(adjust_lr_fn, rows, cols):
        """adjusted_lr / lr (torch/optim/_muon.py _adjust_lr)."""
        if adjust_lr_fn is None or adjust_lr_fn == "original":
            return math.sqrt(max(1, rows / cols))
        if adjust_lr_fn == "match_rms_adamw":
            return 0.2 * math.sqrt(max(rows, cols))
        return 1.0

    P = _ArenaOptimizer.P
    G = _ArenaOptimizer.G

    @property
    def B(self):
        """The momentum buffer [K, ld] (the Muon matrices' spans are used)."""
        return self._B

    def _bind_state(self):
        for k, ps in enumerate(self._mats):
            for p, s in zip(ps, self._slots):
                self.state[p] = {"momentum_buffer": self._B[k, s[0]:s[0] + s[1] * s[2]].view(p.shape)}

    def state_dict(self):
        sd = super().state_dict()  # a `step` tensor of its own per parameter (ArenaAdam.state_dict)
        sd["state"] = {i: ({**st, "step": st["step"].clone()} if "step" in st else st)
                       for i, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """An ArenaMuon or MuonAdamW state dict of the same parameters: the Muon
        group's hyper-parameters are taken over and its momentum buffers copied
        into the flat buffer (state[p] keeps pointing at its views; a matrix
        without an entry starts from zero), the AdamW group goes through
        ArenaAdam.load_state_dict.  torch's Optimizer.load_state_dict is not
        used for the Muon group: it would re-point state[p] at loose tensors."""
        groups, saved = state_dict["param_groups"], state_dict["state"]
        mine = [len(g["params"]) for g in self.param_groups]
        if [len(g["params"]) for g in groups] != mine:
            raise ValueError(f"ArenaMuon.load_state_dict: parameter groups of {mine} parameters expected, got "
                             f"{[len(g['params']) for g in groups]}")
        with torch.no_grad():
            self._B.zero_()
            for p, i in zip(self.param_groups[0]["params"], groups[0]["params"]):
                buf = saved.get(i, {}).get("momentum_buffer")
                if buf is not None:
                    self.state[p]["momentum_buffer"].copy_(buf)
        self.param_groups[0].update({k: v for k, v in groups[0].items() if k != "params"})
        if self.adam is not None:
            ids = groups[1]["params"]
            self.adam.load_state_dict({"state": {j: saved[i] for j, i in enumerate(ids) if i in saved},
                                       "param_groups": [{**groups[1], "params": list(range(len(ids)))}]})
            self.param_groups[1] = self.adam.param_groups[0]
            self.state.update(self.adam.state)
            self.adam.state = self.state

    def _plan(self, present):
        plan = self._plans.pop(present, None)
        if plan is None:
            plan = MuonPlan(self._slots, present, self.P.device)
            while len(self._plans) >= MUON_PLAN_CACHE:  # the least recently used set goes
                del self._plans[next(iter(self._plans))]
        self._plans[present] = plan  # most recently used last
        return plan

    def _muon_pass(self, k, plan, clip):
        g = self.param_groups[0]
        lr, wd, mom, ns = float(g["lr"]), float(g["weight_decay"]), float(g["momentum"]), int(g["ns_steps"])
        a, b, c = (float(v) for v in g["ns_coefficients"])
        ws = self.workspace
        ops.muon_prepare(plan.prep, plan.mats, self.G[k], self._B[k], ws, plan.partials, momentum=mom,
                         one_m_momentum=1 - mom, nesterov=g["nesterov"], clip_coef=clip)
        ops.muon_scale(plan.mats, plan.partials, g["eps"], plan.scale)
        for it in range(ns):
            first = plan.scale if it == 0 else None  # the first iteration carries the normalisation
            for T, sym, _ in plan.classes:
                ops.muon_gemm(ops.MUON_GRAM, T, sym, plan.mats, ws, 0, 0.0, 1.0, first)
            for T, sym, _ in plan.classes:
                ops.muon_gemm(ops.MUON_POLY, T, sym, plan.mats, ws, 0, b, c)
            for T, _, upd in plan.classes:
                ops.muon_gemm(ops.MUON_UPDATE, T, upd, plan.mats, ws, it & 1, a, 1.0, first)
        ops.muon_apply(plan.prep, plan.mats, self.P[k], ws, ns & 1, lr=lr, wd_factor=1 - lr * wd,
                       scale=plan.scale if ns == 0 else None)

    @torch.no_grad()
    def step(self, closure=None, max_norm=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for ar in self.arenas:
            ar.sync_grads()
        present = [tuple(i for i, p in enumerate(ps) if p.grad is not None) for ps in self._mats]
        rest = self.adam is not None and any(p.grad is not None for p in self.adam.param_groups[0]["params"])
        if not rest and not any(present):
            return loss
        clip = None
        if max_norm:  # one coefficient per replica over its whole gradient row
            ops.grad_clip_coef(self.G, self.ld, max_norm, self._partials, self._clip)
            clip = self._clip
        for k, here in enumerate(present):
            if here:
                self._muon_pass(k, self._plan(here), clip[2 * k:2 * k + 2] if clip is not None else None)
        if rest:
            self.adam.step(clip=clip)
            self.placement = self.adam.placement
        return loss


def fusable_muon(spec_cls, kwargs, arena):
    """True when OptimSpec(spec_cls, **kwargs) can run as ArenaMuon on this arena:
    MuonAdamW on an fp32 arena with a gradient set, float learning rates."""
    from .strategy.optim import MuonAdamW
    if spec_cls is not MuonAdamW or not _fp32_arena(arena):
        return False
    kw = dict(kwargs or {})
    return not any(isinstance(kw.get(k), torch.Tensor) for k in ("lr", "adamw_lr"))


_ADAFACTOR_KW = ("lr", "beta2_decay", "eps", "d", "weight_decay")
# torch.optim.Adafactor specs run as ArenaAdafactor: faster than torch's step in every alternated
# pair at K = 1 and K = 8 (profiles/inner_adafactor.txt); False keeps them on torch
ADAFACTOR_FUSED_DEFAULT = True
ADAFACTOR_PLAN_CACHE = 8  # present sets whose device tables an ArenaAdafactor keeps (least recently used evicted)


def fusable_adafactor(spec_cls, kwargs, arena):
    """True when OptimSpec(spec_cls, **kwargs) can run as ArenaAdafactor on this arena:
    torch.optim.Adafactor on an fp32 arena with a gradient set, no maximize, a float
    learning rate, and no tensor of more than two dimensions (torch factors the last
    two dimensions of an N-D tensor batch-wise; that is not built)."""
    if spec_cls is not getattr(torch.optim, "Adafactor", None) or not _fp32_arena(arena):
        return False
    kw = dict(kwargs or {})
    if kw.get("maximize") or set(kw) - (set(_ADAFACTOR_KW) | {"foreach", "maximize"}):
        return False
    if isinstance(kw.get("lr", 1e-2), torch.Tensor):
        return False
    return all(len(s) <= 2 for s in arena.layout.shapes)


def adafactor_slots(shapes, offsets):
    """What is fixed for an arena layout whichever tensors are present.  Per tensor
    (None for an empty one) the dict of its tensor-table fields but the job range: a
    2-D tensor is a matrix of rt x ct tiles whose state is row_var [rows] then col_var
    [cols]; any other a vector of rt chunks whose state is its variance.  Returns
    (slots, state row length, work row length, jobs of all tensors): the work row
    holds every tensor's partials and scalars and, behind them, psq and usq for
    that many jobs."""
    TR, TC = ADAFACTOR_TILE
    slots, st, wk, jobs = [], 0, 0, 0
    for shape, off in zip(shapes, offsets):
        n = math.prod(shape)
        if n == 0:
            slots.append(None)
            continue
        if len(shape) == 2:
            rows, cols = shape
            s = dict(off=off, rows=rows, cols=cols, matrix=1, state=st, rt=-(-rows // TR), ct=-(-cols // TC))
            st += _round_up(rows + cols, 4)
        else:
            s = dict(off=off, rows=1, cols=n, matrix=0, state=st, rt=-(-n // ADAFACTOR_CHUNK), ct=1)
            st += _round_up(n, 4)
        s["rowpart"], s["colpart"] = wk, wk + s["ct"] * s["rows"] * s["matrix"]
        s["scal"] = s["colpart"] + s["rt"] * s["cols"] * s["matrix"]
        wk = s["scal"] + 4
        jobs += s["rt"] * s["ct"]
        slots.append(s)
    return slots, max(st, 4), wk + 2 * jobs, jobs


def adafactor_tables(slots, present, psq0):
    """The tensor table and the job table (lists of rows, include/gym_amd.h
    "Adafactor inner step") of the tensors `present` (indices into slots); psq0: the
    work offset of psq, usq follows it for as many jobs as all slots have."""
    total = sum(s["rt"] * s["ct"] for s in slots if s is not None)
    tens, jobs = [], []
    for t, s in enumerate(slots[i] for i in present):
        job0 = len(jobs)
        jobs += [(t, i, j, 0) for i in range(s["rt"]) for j in range(s["ct"])]
        row = [s["off"], s["rows"], s["cols"], s["matrix"], s["state"], s["rowpart"], s["colpart"], job0,
               len(jobs) - job0, s["rt"], s["ct"], psq0 + job0, psq0 + total + job0, s["scal"]]
        tens.append(row + [0] * (ADAFACTOR_FIELDS - len(row)))
    return tens, jobs


class AdafactorPlan:
    """The device tables of one Adafactor pass over the tensors `present`."""

    def __init__(self, slots, present, psq0, device):
        tens, jobs = adafactor_tables(slots, present, psq0)
        self.tens = torch.tensor(tens, dtype=torch.int64).reshape(-1, ADAFACTOR_FIELDS).to(device)
        self.jobs = torch.tensor(jobs, dtype=torch.int32).reshape(-1, 4).to(device)


class ArenaAdafactor(_ArenaOptimizer):
    """torch.optim.Adafactor (torch/optim/_adafactor.py, _single_tensor_adafactor) over
    one node's ParamArena or a ReplicaArena whose tensors have at most two dimensions:
    step() is five launches over job tables that cover all K replicas
    (ga_adafactor_stats, reduce, unorm, scale, apply) and, with clipping, one
    ga_grad_clip_coef whose coefficient the first of them applies on the device.  No
    host synchronisation, where torch's step reads two norms back per tensor.

    The state is one fp32 [K, ls] set of row_var + col_var floats per matrix and numel
    per vector, and there is no first moment; state[p] holds `step`, and `row_var`
    [R, 1] and `col_var` [1, C] (or `variance`) as views of it, so state_dict() has
    torch's layout and load_state_dict() takes an ArenaAdafactor or a
    torch.optim.Adafactor state dict.  A parameter whose .grad is None is skipped as
    torch skips it (no decay, no state update, its own `step` does not advance): the
    tables are built for the present set and cached by it, and tensors on different
    counts (beta2t and rho are scalars of a launch) take their passes in turn.  While
    every parameter has had a gradient on every step they share one count tensor."""

    def __init__(self, params, arena, lr=1e-2, beta2_decay=-0.8, eps=(None, 1e-3), d=1.0, weight_decay=0.0,
                 foreach=None, maximize=False, placement=True):
        if isinstance(lr, torch.Tensor) or maximize:
            raise ValueError("ArenaAdafactor: a float lr and no maximize (fusable_adafactor)")
        if not 0.0 <= lr:
            raise ValueError(f"Learning rate should be >= 0 but is: {lr}")
        if not 0.0 >= beta2_decay:
            raise ValueError(f"beta2_decay should be <= 0 but is: {beta2_decay}")
        if eps[0] is not None and not 0.0 <= eps[0]:
            raise ValueError(f"epsilon1 should be >= 0 but is: {eps[0]}")
        if not 0.0 <= eps[1]:
            raise ValueError(f"epsilon2 should be >= 0 but is: {eps[1]}")
        if not 1.0 <= d:
            raise ValueError(f"Clipping threshold d should be >= 1 but is: {d}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"weight_decay should be >= 0 but is: {weight_decay}")
        defaults = dict(lr=lr, beta2_decay=beta2_decay, eps=tuple(eps), d=d, weight_decay=weight_decay,
                        foreach=None, maximize=False)  # foreach: accepted and ignored
        super().__init__(params, defaults, arena)
        layout = self.arenas[0].layout
        shape_at = dict(zip(layout.offsets, layout.shapes))
        owned = [(o, n) for _, o, n in self._spans[0]]
        if any([(o, n) for _, o, n in sp] != owned for sp in self._spans):
            raise ValueError("ArenaAdafactor: every replica must own the same tensors")
        shapes = [shape_at[o] for o, _ in owned]
        if any(len(s) > 2 for s in shapes):
            raise ValueError("ArenaAdafactor: tensors of more than two dimensions are not built (fusable_adafactor)")
        self._slots, self.ls, self.lw, njobs = adafactor_slots(shapes, [o for o, _ in owned])
        self._psq0 = self.lw - 2 * njobs
        dev = self.P.device
        self._S = torch.zeros(self.K, self.ls, dtype=torch.float32, device=dev)  # the state set
        self._W = torch.zeros(self.K, self.lw, dtype=torch.float32, device=dev)  # partials and scalars
        self._slot_of = {id(p): (k, i) for k, sp in enumerate(self._spans) for i, (p, _, _) in enumerate(sp)}
        self._count = [[0.0] * len(owned) for _ in range(self.K)]  # the step count of every tensor
        self._clock = torch.tensor(0.0)  # the one count tensor while all tensors share a count, else None
        self._plans = {}
        for p in self.param_groups[0]["params"]:
            self._bind_state(p, self._clock)
        self.placement = {"placed": False, "why": "no search for Adafactor"}

    @property
    def S(self):
        """The state set [K, ls]: per matrix row_var then col_var, per vector its variance."""
        return self._S

    def state_bytes(self):
        return self._S.numel() * 4

    def _bind_state(self, p, step):
        k, i = self._slot_of[id(p)]
        s = self._slots[i]
        if s is None:
            self.state[p] = {"step": step}
        elif s["matrix"]:
            a, R, C = s["state"], s["rows"], s["cols"]
            self.state[p] = {"step": step, "row_var": self._S[k, a:a + R].view(R, 1),
                             "col_var": self._S[k, a + R:a + R + C].view(1, C)}
        else:
            a = s["state"]
            self.state[p] = {"step": step, "variance": self._S[k, a:a + s["cols"]].view(p.shape)}

    def state_dict(self):
        """torch's layout, every parameter with a `step` tensor of its own."""
        sd = super().state_dict()
        sd["state"] = {i: {**st, "step": st["step"].clone()} for i, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """torch's Optimizer.load_state_dict, then the loaded factors are copied into
        the flat state set and the state is re-pointed at its views.  A parameter
        without an entry starts at step 0 with zero state."""
        super().load_state_dict(state_dict)
        loaded = {id(p): dict(self.state.get(p, {})) for p in self.param_groups[0]["params"]}
        counts = {i: float(st.get("step", 0.0)) for i, st in loaded.items()}
        self._clock = torch.tensor(next(iter(counts.values()))) if len(set(counts.values())) == 1 else None
        with torch.no_grad():
            self._S.zero_()
            for p in self.param_groups[0]["params"]:
                k, i = self._slot_of[id(p)]
                self._count[k][i] = counts[id(p)]
                self._bind_state(p, self._clock if self._clock is not None else torch.tensor(counts[id(p)]))
                for key in ("row_var", "col_var", "variance"):
                    if key in loaded[id(p)] and key in self.state[p]:
                        self.state[p][key].copy_(loaded[id(p)][key].reshape(self.state[p][key].shape))

    def _plan(self, present):
        plan = self._plans.pop(present, None)
        if plan is None:
            plan = AdafactorPlan(self._slots, present, self._psq0, self.P.device)
            while len(self._plans) >= ADAFACTOR_PLAN_CACHE:  # the least recently used set goes
                del self._plans[next(iter(self._plans))]
        self._plans[present] = plan  # most recently used last
        return plan

    def _advance(self, present):
        """Advance the count of every present tensor; returns per replica {count: the
        present tensors on it}."""
        everything = all(len(pr) == sum(s is not None for s in self._slots) for pr in present)
        if self._clock is not None and everything:
            self._clock += 1  # every tensor present on one count: nothing per parameter
            t = float(self._clock)
            self._count = [[t] * len(c) for c in self._count]
            return [{t: pr} for pr in present]
        if self._clock is not None:  # from here on every parameter counts for itself
            for p in self.param_groups[0]["params"]:
                self.state[p]["step"] = self._clock.clone()
            self._clock = None
        groups = []
        for k, pr in enumerate(present):
            by_count = {}
            for i in pr:
                self.state[self._spans[k][i][0]]["step"] += 1
                self._count[k][i] += 1.0
                by_count.setdefault(self._count[k][i], []).append(i)
            groups.append({t: tuple(idx) for t, idx in by_count.items()})
        return groups

    def _pass(self, k, t, present, clip):
        """The five launches for the tensors `present`, all on count t, of replica k (None: of every replica)."""
        g = self.param_groups[0]
        lr, wd, (eps1, eps2) = float(g["lr"]), float(g["weight_decay"]), g["eps"]
        eps1 = torch.finfo(torch.float32).eps if eps1 is None else float(eps1)
        beta2t, rho = t ** float(g["beta2_decay"]), min(lr, 1 / math.sqrt(t))
        plan = self._plan(present)
        P, G, S, W = ((x if k is None else x[k:k + 1]) for x in (self.P, self.G, self._S, self._W))
        if clip is not None and k is not None:
            clip = clip[2 * k:2 * k + 2]
        ops.adafactor_stats(plan.jobs, plan.tens, P, G, S, W, beta2t=beta2t, clip_coef=clip)
        ops.adafactor_reduce(plan.tens, S, W, beta2t=beta2t, rho=rho, eps1=eps1, eps2=float(eps2))
        ops.adafactor_unorm(plan.jobs, plan.tens, G, S, W, eps1=eps1)
        ops.adafactor_scale(plan.tens, W, d=float(g["d"]))
        ops.adafactor_apply(plan.jobs, plan.tens, P, G, S, W, eps1=eps1,
                            wd_factor=(1 - lr * wd) if wd != 0 else 1.0)

    @torch.no_grad()
    def step(self, closure=None, max_norm=None, clip=None):
        """clip: the coefficients of a ga_grad_clip_coef the caller already ran over the gradient set."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for ar in self.arenas:
            ar.sync_grads()
        present = [tuple(i for i, (p, _, _) in enumerate(sp) if p.grad is not None and self._slots[i] is not None)
                   for sp in self._spans]
        if not any(present):  # no parameter has a gradient: torch's step does nothing
            return loss
        groups = self._advance(present)
        if clip is None and max_norm:
            ops.grad_clip_coef(self.G, self.ld, max_norm, self._partials, self._clip)
            clip = self._clip
        if all(g == groups[0] for g in groups):  # one launch set covers the K rows
            for t, idx in groups[0].items():
                self._pass(None, t, idx, clip)
        else:
            for k, by_count in enumerate(groups):
                for t, idx in by_count.items():
                    self._pass(k, t, idx, clip)
        return loss


FUSED = (ArenaAdam, ArenaAdam8bit, ArenaSGD, ArenaMuon, ArenaAdafactor)  # the inner optimizers whose step(max_norm=) clips on the device


def build_fused(spec, params, arena, placement=True, models=None):
    """The fused inner optimizer of OptimSpec `spec` over `arena` (ArenaAdam for
    torch's AdamW / Adam, ArenaSGD for torch's SGD, ArenaAdafactor for torch's
    Adafactor under ADAFACTOR_FUSED_DEFAULT, ArenaAdam8bit for AdamW8bit, ArenaMuon for MuonAdamW with
    `fused=True` -- MUON_FUSED_DEFAULT without the kwarg), or None when the spec
    stays on torch: another optimizer or option, a bf16 arena, or
    GA_FUSED_OPTIM=0.  models: the arena's modules (one per replica), from which
    a MuonAdamW spec selects its matrices."""
    import os
    if os.environ.get("GA_FUSED_OPTIM", "1") == "0":
        return None
    kw = spec.kwargs or {}
    if fusable_muon(spec.cls, kw, arena):
        fused = kw.get("fused")
        if not (MUON_FUSED_DEFAULT if fused is None else fused):
            return None
        from .strategy.optim import muon_matrix_mask
        mask = kw.get("muon_mask")
        if mask is None:
            if not models:
                return None
            mask = muon_matrix_mask(models[0], kw.get("muon_exclude", ("lm_head",)), kw.get("muon_params"))
        if not any(mask):
            return None
        opt = ArenaMuon(list(params), arena, mask, placement=placement,
                        **{k: v for k, v in kw.items() if k not in ("muon_mask", "muon_exclude", "muon_params",
                                                                    "fused")})
        names = [n for n, _ in models[0].named_parameters()] if models else [str(i) for i in range(len(mask))]
        opt.muon_names = [n for n, m in zip(names, mask) if m]
        return opt
    if fusable(spec.cls, kw, arena):
        kw = {k: v for k, v in kw.items() if k in ("lr", "betas", "eps", "weight_decay")}
        return ArenaAdam(params, arena, decoupled=spec.cls is torch.optim.AdamW, placement=placement, **kw)
    # a stand-in kernel layer (tests) written before ga_sgd_step keeps torch's SGD; gym_amd.ops always has it
    if fusable_sgd(spec.cls, kw, arena) and hasattr(ops, "sgd_step"):
        return ArenaSGD(params, arena, placement=placement, **{k: v for k, v in kw.items() if k in _SGD_KW})
    # likewise a stand-in layer written before ga_adafactor_* keeps torch's Adafactor
    if ADAFACTOR_FUSED_DEFAULT and fusable_adafactor(spec.cls, kw, arena) and hasattr(ops, "adafactor_stats"):
        return ArenaAdafactor(params, arena, placement=placement,
                              **{k: v for k, v in kw.items() if k in _ADAFACTOR_KW})
    # and one written before ga_adam8_step keeps the unfused AdamW8bit
    if fusable_adam8(spec.cls, kw, arena) and hasattr(ops, "adam8_step"):
        return ArenaAdam8bit(params, arena, placement=placement, **kw)
    return None
