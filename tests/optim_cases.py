"""Shared cases for the fused inner optimizer tests (CPU stand-ins and GPU):
ArenaAdam vs torch.optim.AdamW / Adam (+ clip_grad_norm_) on the same model,
gradients and steps.  torch's optimizer is the reference's inner optimizer
(exogym/strategy/optim.py:11, strategy.py:135-140).

A presence pattern says on which steps a parameter has no gradient (.grad is
None at step time); torch then leaves the parameter, its moments and its own
`step` alone, and so must ArenaAdam."""
import numpy as np
import torch

SHAPES = [(66, 32), (128,), (96, 64), (3, 7), (10,)]
ALL = frozenset(range(64))  # absent on every step
PATTERN_STEPS = 6


def make_model(dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    m = torch.nn.Module()
    m.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, generator=g) * 0.02) for s in SHAPES])
    return m.to(dev)


def grads_for(step, seed=7):
    g = torch.Generator().manual_seed(seed + 31 * step)
    return [torch.randn(*s, generator=g) * (0.05 if step % 2 else 0.5) for s in SHAPES]


def warmup(step):
    """The LambdaLR factor of the warm-up case (the scheduler's own step count)."""
    return min(1.0, (step + 1) / 4)


class Pattern:
    """absent: {parameter index: steps on which its .grad is None}; frozen:
    indices with requires_grad False (in the optimizer's list all the same);
    sched: a LambdaLR warm-up drives lr."""

    def __init__(self, absent=None, frozen=(), sched=False):
        self.absent = {i: frozenset(s) for i, s in (absent or {}).items()}
        self.frozen = tuple(frozen)
        self.sched = sched

    def present(self, i, step):
        return i not in self.frozen and step not in self.absent.get(i, ())


def _pattern(skip, pattern):
    if pattern is not None:
        return pattern
    if skip is not None:  # the parameter's grad is None from step 2 on
        return Pattern({skip: range(2, 64)})
    return Pattern()


def _state(opt, params):
    """torch's layout, as host arrays; a parameter without state reports step 0 and zero moments."""
    out = {"params": [p.detach().cpu().numpy().copy() for p in params], "exp_avg": [], "exp_avg_sq": [], "step": []}
    for p in params:
        st = opt.state.get(p, {})
        for key in ("exp_avg", "exp_avg_sq"):
            out[key].append(st[key].detach().cpu().numpy().copy() if key in st else np.zeros(p.shape, np.float32))
        out["step"].append(float(st["step"]) if "step" in st else 0.0)
    return out


def run_pair(dev, cls, kw, max_norm=None, steps=5, skip=None, pattern=None, K=1, observe=None, slack=0):
    """(ours, torch's) after `steps` steps, each {"params", "exp_avg",
    "exp_avg_sq", "step"}: per-parameter lists (replica-major for K > 1).
    `skip` = index of a parameter whose grad is None from step 2 on; `pattern` =
    a Pattern, or for K > 1 a list of one per replica (ArenaAdam over a
    ReplicaArena against K independent torch optimizers, each replica with its
    own model, gradients and clipping).  observe(when, step, ctx), when in
    ("before", "after") of ArenaAdam's step: ctx has arena, opt, models, pats."""
    from gym_amd.arena import ParamArena, ReplicaArena
    from gym_amd.fused_optim import ArenaAdam
    pats = pattern if isinstance(pattern, (list, tuple)) else [_pattern(skip, pattern)] * K
    ours_m = [make_model(dev, seed=3 + k) for k in range(K)]
    ref_m = [make_model(dev, seed=3 + k) for k in range(K)]
    for pat, a, b in zip(pats, ours_m, ref_m):
        for i in pat.frozen:
            a.ps[i].requires_grad_(False)
            b.ps[i].requires_grad_(False)
    if K == 1:
        arena = ParamArena(list(ours_m[0].parameters()))
        ours = ArenaAdam(ours_m[0].parameters(), arena, decoupled=cls is torch.optim.AdamW, **kw)
    else:
        arena = ReplicaArena(ours_m)
        ours = ArenaAdam(arena.params, arena, decoupled=cls is torch.optim.AdamW, **kw)
    if slack:  # all four sets into buffers with `slack` elements behind the last row, for the GPU sentinels
        ld = ours.ld
        P, G, M, V = (torch.zeros(K * ld + slack, device=dev)[:K * ld].view(K, ld) for _ in range(4))
        if K == 1:
            arena.relocate(P[0], G[0])
        else:
            arena.relocate_params(P)
            arena.relocate_grads(G)
        ours.move_moments(M, V)
    refs = [cls(b.parameters(), **kw) for b in ref_m]
    scheds = []
    if pats[0].sched:
        scheds = [torch.optim.lr_scheduler.LambdaLR(o, warmup) for o in [ours] + refs]
    ctx = {"arena": arena, "opt": ours, "models": ours_m, "pats": pats, "dev": dev}
    for step in range(steps):
        arena.zero_grad()
        for k, (pat, a, b) in enumerate(zip(pats, ours_m, ref_m)):
            for i, (pa, pb, g) in enumerate(zip(a.parameters(), b.parameters(), grads_for(step, seed=7 + 1000 * k))):
                if not pat.present(i, step):
                    pa.grad = None
                    pb.grad = None
                    continue
                pa.grad.copy_(g.to(dev))
                pb.grad = g.to(dev).clone()
        if observe is not None:
            observe("before", step, ctx)
        ours.step(max_norm=max_norm)
        if observe is not None:
            observe("after", step, ctx)
        for b, ref in zip(ref_m, refs):
            if max_norm:
                torch.nn.utils.clip_grad_norm_([p for p in b.parameters() if p.grad is not None], max_norm)
            ref.step()
        for s in scheds:
            s.step()
    mine = _state(ours, [p for a in ours_m for p in a.parameters()])
    theirs = [_state(ref, list(b.parameters())) for b, ref in zip(ref_m, refs)]
    return mine, {key: [v for t in theirs for v in t[key]] for key in mine}


_ADAMW = (torch.optim.AdamW, {"lr": 1e-2})
_ADAM_L2 = (torch.optim.Adam, {"lr": 1e-2, "weight_decay": 0.05})
_EVERY = range(len(SHAPES))

PATTERNS = [
    ("late-start", Pattern({1: (0, 1)})),
    ("gap", Pattern({1: (2, 3)})),
    ("never", Pattern({1: ALL})),
    ("frozen", Pattern({4: (2, 3)}, frozen=(2,))),
    # tensors 0 and 2 on counts of their own with a present tensor between them
    ("two-counts", Pattern({0: (0,), 2: (0, 1)})),
    ("empty-step", Pattern({i: (2,) for i in _EVERY})),  # step 2: nothing has a gradient
    # (3, 7) and (10,), numel % 4 != 0, each the last tensor of a range: before an absent one, and alone
    ("tail", Pattern({4: (2, 3), 3: (4,), 2: (4,)})),
]

# (name, optimizer class, its kwargs, max_norm, skip, pattern)
CASES = [
    ("adamw-default", torch.optim.AdamW, {}, None, None, None),
    ("adamw-wd-lr", torch.optim.AdamW, {"lr": 3e-3, "weight_decay": 0.1, "betas": (0.8, 0.95)}, None, None, None),
    ("adamw-clip", torch.optim.AdamW, {"lr": 1e-3}, 0.5, None, None),
    ("adam-l2", torch.optim.Adam, {"lr": 2e-3, "weight_decay": 0.05}, None, None, None),
    ("adamw-unused-param", torch.optim.AdamW, {"lr": 1e-3}, None, 1, None),
    ("adamw-beta1-small", torch.optim.AdamW, {"lr": 1e-3, "betas": (0.3, 0.9)}, None, None, None),  # lerp weight >= 0.5
    ("adamw-clip-unused-param", torch.optim.AdamW, {"lr": 1e-3}, 0.5, 1, None),
]
PATTERN_CASES = [(f"{oname}-{pname}{'-clip' if mn else ''}", cls, kw, mn, None, pat)
                 for pname, pat in PATTERNS
                 for oname, (cls, kw) in (("adamw", _ADAMW), ("adam-l2", _ADAM_L2))
                 for mn in (None, 0.5)]
PATTERN_CASES.append(("adamw-gap-warmup", torch.optim.AdamW, {"lr": 1e-2}, 0.5, None, Pattern({1: (2, 3)}, sched=True)))
CASES = CASES + PATTERN_CASES

# K = 3 replicas of one ReplicaArena, a different pattern on each: the ranges, the clip
# slices and the counts all differ per row
REPLICA_PATTERNS = [Pattern({1: (0, 1)}), Pattern({0: (0,), 2: (0, 1), 4: (2, 3)}), Pattern({3: ALL, 1: (2, 3)})]
REPLICA_CASES = [(f"{oname}-replicas{'-clip' if mn else ''}", cls, kw, mn)
                 for oname, (cls, kw) in (("adamw", _ADAMW), ("adam-l2", _ADAM_L2)) for mn in (None, 0.5)]


def case_steps(pattern):
    return PATTERN_STEPS if pattern is not None else 5


def assert_close(ours, ref, rtol=1e-5, atol=1e-7):
    """Parameters (a list of arrays), or the dicts of run_pair: parameters and
    both moments within the tolerance, every parameter's `step` exactly."""
    if isinstance(ours, dict):
        for key in ("params", "exp_avg", "exp_avg_sq"):
            for i, (x, y) in enumerate(zip(ours[key], ref[key])):
                np.testing.assert_allclose(x, y, rtol=rtol, atol=atol, err_msg=f"{key}[{i}]")
        assert ours["step"] == ref["step"], (ours["step"], ref["step"])
        return
    for x, y in zip(ours, ref):
        np.testing.assert_allclose(x, y, rtol=rtol, atol=atol)
