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
per-parameter initialised flag where Adam has a step count.  build_fused picks
the class for a spec; FUSED names both for the callers that step them.
"""
import math
import time

import torch

from . import ops

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
            if len(out) == 1 and len(spans) == len(self._spans[k]):
                out = [[0, self.ld, out[0][2]]]
            ranges.append([tuple(r) for r in out])
        return ranges

    _whole_set = True  # one launch may cover the [K, ld] sets when every replica has the same whole-row range

    def _finish(self):
        pass

    @torch.no_grad()
    def step(self, closure=None, max_norm=None):
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
        clip = None
        if max_norm:
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


class ArenaAdam(_ArenaOptimizer):
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
        # the step counts: [count tensor, [(param, replica, offset, numel)]] per group of parameters that
        # share a count -- state[p]["step"] of its members IS the group's tensor, so a step advances a
        # group with one add.  One group while every parameter has had a gradient on every step.
        self._groups = [[torch.tensor(0.0), []]]
        for p in self.param_groups[0]["params"]:
            self._groups[0][1].append((p, *self._where[id(p)]))
            self._bind_state(p)
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

    def state_dict(self):
        """torch's layout, every parameter with a `step` tensor of its own (here
        the parameters of a group share one; torch's optimizers, which advance
        each entry in place, must not)."""
        sd = super().state_dict()
        sd["state"] = {i: {**st, "step": st["step"].clone()} for i, st in sd["state"].items()}
        return sd

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
        groups = {}  # one group, and one count tensor, per distinct count
        for k, sp in enumerate(self._spans):
            for p, o, n in sp:
                t = steps[id(p)]
                g = groups.get(t) or groups.setdefault(t, [torch.tensor(t), []])
                g[1].append((p, k, o, n))
                self.state[p]["step"] = g[0]
                self._bind_state(p)
        self._groups = list(groups.values())

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

    def _ranges(self):
        """Advance the count of every parameter that has a gradient now and
        return, per replica, [(a, b, t)]: the contiguous ranges of present
        parameters that share the count t (_join).  A group whose members
        are all present advances with one add; one that is partly present
        splits; groups that reach the same count become one again."""
        groups = self._groups
        if len(groups) == 1 and all(m[0].grad is not None for m in groups[0][1]):
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
        g = self.param_groups[0]
        lr, (b1, b2), eps, wd = float(g["lr"]), g["betas"], float(g["eps"]), float(g["weight_decay"])
        decoupled = g["decoupled_weight_decay"]
        bc1 = 1 - b1 ** t
        bc2 = 1 - b2 ** t
        return dict(lerp_w=1 - b1, beta2=b2, one_m_beta2=1 - b2, eps=eps,
                    wd_factor=(1 - lr * wd) if (decoupled and wd != 0) else 1.0,
                    l2_wd=wd if (not decoupled and wd != 0) else 0.0, step_size=-(lr / bc1), bc2_sqrt=math.sqrt(bc2))


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


FUSED = (ArenaAdam, ArenaSGD)  # the inner optimizers whose step(max_norm=) clips on the device


def build_fused(spec, params, arena, placement=True):
    """The fused inner optimizer of OptimSpec `spec` over `arena` (ArenaAdam for
    torch's AdamW / Adam, ArenaSGD for torch's SGD), or None when the spec stays
    on torch: another optimizer or option, a bf16 arena, or GA_FUSED_OPTIM=0."""
    import os
    if os.environ.get("GA_FUSED_OPTIM", "1") == "0":
        return None
    kw = spec.kwargs or {}
    if fusable(spec.cls, kw, arena):
        kw = {k: v for k, v in kw.items() if k in ("lr", "betas", "eps", "weight_decay")}
        return ArenaAdam(params, arena, decoupled=spec.cls is torch.optim.AdamW, placement=placement, **kw)
    # a stand-in kernel layer (tests) written before ga_sgd_step keeps torch's SGD; gym_amd.ops always has it
    if fusable_sgd(spec.cls, kw, arena) and hasattr(ops, "sgd_step"):
        return ArenaSGD(params, arena, placement=placement, **{k: v for k, v in kw.items() if k in _SGD_KW})
    return None
