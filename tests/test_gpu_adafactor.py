"""The fused Adafactor inner step (ArenaAdafactor through build_fused: ga_adafactor_stats / reduce /
unorm / scale / apply) against torch.optim.Adafactor(foreach=False) on float64 CPU copies of the same
parameters and the same (identically clipped) gradients.

Shapes, by the boundary they hit (tile 64 x 256, vector chunk 4096): a matrix under one tile, exactly
one, one plus one in both directions (cols % 4 != 0: the scalar path), several ragged tiles, a tall
matrix of 3 columns, a single row, and the vector path down to 0-d.  Row 2 of every gradient with
more than 4 rows is zero (the eps1^2 clamp is live); magnitudes differ per tensor by 10^(i mod 3 - 1).

Gate: with err(x) = max|x - x64| / max|x64|, every parameter and every row_var, col_var and variance
after every step holds err_fused <= max(4 err_torch32, 32 * 2^-24), err_torch32 the same error of
torch's own fp32 Adafactor on the GPU on the same inputs: both are fp32 and differ in the order of
sums and in FMA contraction; the floor allows a chain of about 16 rounded operations plus blocked
sums over at most 2^17 terms."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7), (64, 256), (65, 257), (130, 515), (515, 3), (1, 300), (1000,), (63,), (1,), ()]
ABSENT = 2  # the 65 x 257 matrix of replica 0 has no gradient on the second step
EPS = (float(torch.finfo(torch.float32).eps), 1e-3)
FLOOR = 32 * 2.0 ** -24
SLACK = 64
GROW = dict(factor=3.0, lr=0.5, weight_decay=0.1)      # the update clip max(1, RMS(u) / d) is active
SHRINK = dict(factor=1 / 3, lr=1e-2, weight_decay=0.0)  # and inactive


class Bag(torch.nn.Module):
    def __init__(self, seed, zero):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.randn(s, generator=g) * (0.0 if zero else 0.05)) for s in SHAPES])


def _grads(step, k, factor):
    rng = np.random.default_rng([7, step, k])
    out = []
    for i, s in enumerate(SHAPES):
        g = rng.standard_normal(s) * 10.0 ** (i % 3 - 1) * factor ** step
        if len(s) == 2 and s[0] > 4:
            g[2] = 0.0
        out.append(torch.from_numpy(np.asarray(g, dtype=np.float32)))
    return out


def _setup(K, mode, zero):
    """K replicas of the bag in a ReplicaArena whose parameter set has 64 sentinel elements behind
    the last row, and the fused optimizer build_fused gives for the spec."""
    from gym_amd.arena import ReplicaArena
    from gym_amd.fused_optim import ArenaAdafactor, build_fused
    from gym_amd.strategy.optim import OptimSpec
    dev = torch.device("cuda:0")
    models = [Bag(5 + k, zero).to(dev) for k in range(K)]
    ra = ReplicaArena(models)
    big = torch.full((K * ra.ld + SLACK,), 7.0, device=dev)
    big[:K * ra.ld] = 0
    ra.relocate_params(big[:K * ra.ld].view(K, ra.ld))
    spec = OptimSpec.from_string("adafactor", lr=mode["lr"], weight_decay=mode["weight_decay"], eps=EPS)
    opt = build_fused(spec, ra.params, ra, models=models)
    assert isinstance(opt, ArenaAdafactor)
    return models, ra, big, opt


def _fused_step(models, ra, opt, t, mode, max_norm, absent):
    """Step t of the fused optimizer.  Returns per replica the gradients it used (the clipped ones it
    wrote back; None for the absent matrix) after checking them bitwise against g * coef."""
    ra.zero_grad()
    raw = [[g.cuda() for g in _grads(t, k, mode["factor"])] for k in range(len(models))]
    gone = lambda k, i: absent and t == 1 and k == 0 and i == ABSENT  # noqa: E731
    for k, (m, gs) in enumerate(zip(models, raw)):
        for i, (p, g) in enumerate(zip(m.parameters(), gs)):
            if gone(k, i):
                p.grad = None
            else:
                p.grad.copy_(g)
    opt.step(max_norm=max_norm)
    used = []
    for k, gs in enumerate(raw):
        coef = opt._clip[2 * k] if max_norm else None
        assert coef is None or float(coef) < 1.0  # max_norm is small enough to clip
        views = ra.layout.views(ra.grad_set[k])
        used.append([None if gone(k, i) else v.clone() for i, v in enumerate(views)])
        for i, (g, v) in enumerate(zip(gs, used[-1])):
            assert v is None or torch.equal(v, g * coef if max_norm else g), (k, i)
    return used


def _err(x, x64):
    diff, den = float((x.double().cpu() - x64).abs().max()), float(x64.abs().max())
    return diff / den if den else (0.0 if diff == 0 else float("inf"))


def _gate(what, fused, t32, ref, worst):
    if not torch.is_tensor(ref):  # a parameter's state: its factors
        for key in ("row_var", "col_var", "variance"):
            if key in ref:
                _gate(f"{what}.{key}", fused[key], t32[key], ref[key], worst)
        return
    ef, et = _err(fused, ref), _err(t32, ref)
    worst[0], worst[1] = max(worst[0], ef / max(et, FLOOR / 4)), max(worst[1], ef)
    assert ef <= max(4 * et, FLOOR), (what, ef, et)


CASES = [  # K, gradients and hyper-parameters, zero-initialised parameters, max_norm, ABSENT absent on step 2
    (1, GROW, False, None, False), (3, GROW, False, 1.0, True), (1, SHRINK, True, None, False),
    (3, SHRINK, False, 1.0, False), (1, GROW, True, 1.0, True)]


@pytest.mark.parametrize("K,mode,zero,max_norm,absent", CASES)
def test_fused_adafactor_step(K, mode, zero, max_norm, absent):
    models, ra, big, opt = _setup(K, mode, zero)
    kw = dict(lr=mode["lr"], weight_decay=mode["weight_decay"], eps=EPS, foreach=False)
    ref = [[torch.nn.Parameter(p.detach().double().cpu()) for p in m.parameters()] for m in models]
    t32 = [[torch.nn.Parameter(p.detach().clone()) for p in m.parameters()] for m in models]
    ref_opt = [torch.optim.Adafactor(ps, **kw) for ps in ref]
    t32_opt = [torch.optim.Adafactor(ps, **kw) for ps in t32]
    pad = np.ones(ra.ld, bool)
    for o, n in zip(ra.layout.offsets, ra.layout.numels):
        pad[o:o + n] = False
    pad = np.concatenate([np.tile(pad, K), np.ones(SLACK, bool)])
    before, worst = big.cpu().numpy().copy(), [0.0, 0.0]
    for t in range(3):
        skipped = [list(m.parameters())[ABSENT].detach().clone() for m in models]
        used = _fused_step(models, ra, opt, t, mode, max_norm, absent)
        for k, m in enumerate(models):
            for plist, o in ((ref[k], ref_opt[k]), (t32[k], t32_opt[k])):
                for p, g in zip(plist, used[k]):
                    p.grad = None if g is None else g.to(p.device, p.dtype)
                o.step()
            for i, p in enumerate(m.parameters()):
                _gate(f"step {t} replica {k} {SHAPES[i]}", p.detach(), t32[k][i].detach(), ref[k][i].detach(), worst)
                _gate(f"step {t} replica {k} {SHAPES[i]}", opt.state[p], t32_opt[k].state[t32[k][i]],
                      ref_opt[k].state[ref[k][i]], worst)
                assert float(opt.state[p]["step"]) == float(ref_opt[k].state[ref[k][i]]["step"])
            if absent and t == 1 and k == 0:  # skipped exactly, and its own count stays
                p = list(m.parameters())[ABSENT]
                assert torch.equal(p.detach(), skipped[k]) and float(opt.state[p]["step"]) == 1.0
    print(f"adafactor K={K} lr={mode['lr']} zero={zero} max_norm={max_norm} absent={absent}: "
          f"worst err_fused / max(err_torch32, floor / 4) = {worst[0]:.3f}, worst err_fused = {worst[1]:.3g}")
    after = big.cpu().numpy()
    assert np.array_equal(before[pad], after[pad]) and (after[-SLACK:] == 7.0).all()
    # determinism: every sum has a fixed order, the same bits twice
    models2, ra2, big2, opt2 = _setup(K, mode, zero)
    for t in range(3):
        _fused_step(models2, ra2, opt2, t, mode, max_norm, absent)
    assert torch.equal(big, big2) and torch.equal(opt.S, opt2.S)


def test_resumes_from_a_torch_adafactor_state_dict():
    """Two steps of torch's fp32 Adafactor, its state dict loaded into ArenaAdafactor, one fused step."""
    models, ra, _, opt = _setup(1, GROW, False)
    kw = dict(lr=GROW["lr"], weight_decay=GROW["weight_decay"], eps=EPS, foreach=False)
    ref = [torch.nn.Parameter(p.detach().double().cpu()) for p in models[0].parameters()]
    t32 = [torch.nn.Parameter(p.detach().clone()) for p in models[0].parameters()]
    ref_opt, t32_opt = torch.optim.Adafactor(ref, **kw), torch.optim.Adafactor(t32, **kw)
    for t in range(3):
        if t == 2:
            with torch.no_grad():
                for p, q in zip(models[0].parameters(), t32):
                    p.copy_(q)
            opt.load_state_dict(t32_opt.state_dict())
            used = _fused_step(models, ra, opt, t, GROW, None, False)[0]
        for plist, o in ((ref, ref_opt), (t32, t32_opt)):
            for p, g in zip(plist, _grads(t, 0, GROW["factor"])):
                p.grad = g.to(p.device, p.dtype)
            o.step()
    worst = [0.0, 0.0]
    for i, p in enumerate(models[0].parameters()):
        assert torch.equal(used[i], _grads(2, 0, GROW["factor"])[i].cuda())
        st = opt.state[p]
        assert float(st["step"]) == 3.0
        key = "row_var" if len(SHAPES[i]) == 2 else "variance"
        assert st[key].untyped_storage().data_ptr() == opt.S.untyped_storage().data_ptr()
        _gate(f"resumed {SHAPES[i]}", p.detach(), t32[i].detach(), ref[i].detach(), worst)
        _gate(f"resumed {SHAPES[i]}", st, t32_opt.state[t32[i]], ref_opt.state[ref[i]], worst)
