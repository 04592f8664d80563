"""Shared cases for the fused SGD inner optimizer tests (CPU stand-ins and GPU):
ArenaSGD vs torch.optim.SGD (+ clip_grad_norm_) on the same model, gradients
and steps.  torch's SGD is the reference's "sgd" inner optimizer
(exogym/strategy/optim.py:24, strategy.py:135-140).

The models, gradients, presence patterns and tolerance are optim_cases'.  torch
creates a parameter's momentum buffer as a clone of the first gradient it sees,
so the patterns in which a parameter's first gradient comes after its
neighbours' ("late-start", "gap", "two-counts") are the ones where one step
needs launches with different `first` flags."""
import numpy as np
import torch

from optim_cases import (PATTERN_STEPS, PATTERNS, REPLICA_PATTERNS, SHAPES, Pattern, assert_close, grads_for,  # noqa: F401
                         make_model, warmup)

# (name, torch.optim.SGD kwargs)
SETTINGS = [
    ("plain", {"lr": 0.1}),
    ("momentum", {"lr": 0.1, "momentum": 0.9}),
    ("dampening", {"lr": 0.1, "momentum": 0.9, "dampening": 0.9}),
    ("nesterov", {"lr": 0.1, "momentum": 0.9, "nesterov": True}),
    ("l2", {"lr": 0.1, "weight_decay": 0.05}),
    ("l2-momentum", {"lr": 0.1, "momentum": 0.9, "weight_decay": 0.05}),
]

# (name, kwargs, max_norm, pattern): every setting, clipped and not, on every pattern, and once all-present
CASES = [(f"{sname}-{pname}{'-clip' if mn else ''}", kw, mn, pat)
         for sname, kw in SETTINGS for pname, pat in [("all", Pattern())] + PATTERNS for mn in (None, 0.5)]
# a LambdaLR warm-up drives lr, once per setting (tensor 1 absent at steps 2-3)
CASES += [(f"{sname}-gap-warmup", kw, 0.5, Pattern({1: (2, 3)}, sched=True)) for sname, kw in SETTINGS]
REPLICA_CASES = [(f"{sname}-replicas{'-clip' if mn else ''}", kw, mn) for sname, kw in SETTINGS for mn in (None, 0.5)]


def _state(opt, params):
    """Host copies: the parameters, each parameter's momentum buffer (zeros when
    it has none) and whether it has one (torch: an entry in `state`)."""
    out = {"params": [p.detach().cpu().numpy().copy() for p in params], "momentum_buffer": [], "has_buffer": []}
    for p in params:
        b = opt.state.get(p, {}).get("momentum_buffer")
        out["has_buffer"].append(b is not None)
        out["momentum_buffer"].append(b.detach().cpu().numpy().copy() if b is not None else np.zeros(p.shape, np.float32))
    return out


def run_pair(dev, kw, max_norm=None, steps=PATTERN_STEPS, pattern=None, K=1, observe=None, slack=0):
    """(ours, torch's) after `steps` steps, each {"params", "momentum_buffer",
    "has_buffer"}: per-parameter lists (replica-major for K > 1).  pattern: a
    Pattern, or for K > 1 a list of one per replica (ArenaSGD over a
    ReplicaArena against K independent torch optimizers, each replica with its
    own model, gradients and clipping).  observe(when, step, ctx), when in
    ("before", "after") of ArenaSGD's step: ctx has arena, opt, models, pats.
    slack: parameters, gradients and the buffer go into memory with `slack`
    elements behind the last row (the GPU sentinels read them)."""
    from gym_amd.arena import ParamArena, ReplicaArena
    from gym_amd.fused_optim import ArenaSGD
    pats = pattern if isinstance(pattern, (list, tuple)) else [pattern or Pattern()] * K
    ours_m = [make_model(dev, seed=3 + k) for k in range(K)]
    ref_m = [make_model(dev, seed=3 + k) for k in range(K)]
    for pat, a, b in zip(pats, ours_m, ref_m):
        for i in pat.frozen:
            a.ps[i].requires_grad_(False)
            b.ps[i].requires_grad_(False)
    if K == 1:
        arena = ParamArena(list(ours_m[0].parameters()))
        ours = ArenaSGD(ours_m[0].parameters(), arena, **kw)
    else:
        arena = ReplicaArena(ours_m)
        ours = ArenaSGD(arena.params, arena, **kw)
    if slack:
        ld = ours.ld
        P, G, B = (torch.zeros(K * ld + slack, device=dev)[:K * ld].view(K, ld) for _ in range(3))
        if K == 1:
            arena.relocate(P[0], G[0])
        else:
            arena.relocate_params(P)
            arena.relocate_grads(G)
        if kw.get("momentum"):
            ours.move_buffer(B)
    refs = [torch.optim.SGD(b.parameters(), **kw) for b in ref_m]
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


def assert_same(ours, ref):
    """Parameters and momentum buffers within optim_cases.assert_close's project
    tolerance (rtol 1e-5, atol 1e-7), and the same parameters have a buffer."""
    assert ours["has_buffer"] == ref["has_buffer"], (ours["has_buffer"], ref["has_buffer"])
    assert_close(ours["params"], ref["params"])
    assert_close(ours["momentum_buffer"], ref["momentum_buffer"])
