"""The fused 8-bit AdamW step on the MI355X: ga_adam8_step and ga_adam8_encode bit for bit against the
numpy restatement (adam8_checks), ArenaAdam8bit through build_fused in both modes against the torch
class AdamW8bit on the same device and gradients, and a resumed run.

Kernel inputs per row of n elements (ld = n + 128, sentinels behind n): block 0 holds the row's largest
gradient, negative (x / absmax exactly -1 for exp_avg, 1 for exp_avg_sq), beside one of 1e-5 (second
moments > 1e8 apart: the code-1 rule); from three blocks on, block 1 is all zero and block 2 has one
non-zero element; the last 10 elements are zero padding.  Measured (profiles/inner_adam8bit.txt): every
case bit-identical, so no off-by-one allowance; through build_fused d = 0 in both modes, D = 1.46e-3."""
import numpy as np
import pytest
import torch

import adam8_checks as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HP = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8)
KEYS = ("exp_avg_code", "exp_avg_absmax", "exp_avg_sq_code", "exp_avg_sq_absmax")
LONG = 2048 * 1024 + 320  # past one trip of the persistent grid at K = 1


def _row(rng, n, t):
    g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    g[0], g[1] = -5.0 / (t + 1), 1e-5
    if n >= 192:
        g[64:192] = 0
        g[130] = 0.3
    g[n - 10:] = 0
    return g


def _check_step(n, K, decoupled, clip):
    from gym_amd import ops
    from gym_amd.strategy.optim import adam_scalars
    rng = np.random.default_rng([n, K])
    ld, b = n + 128, n // 64
    p0 = (rng.standard_normal((K, n)) * 0.1).astype(np.float32)
    p0[:, n - 10:] = p0[:, 1] = p0[:, 64:192] = 0  # under L2 decay too the special blocks stay what they are
    behind = (7.0, 9.0, 33, 5.0, 44, 6.0)  # sentinels of P, G, Mc, Ma, Vc, Va behind n
    P, G, Mc, Ma, Vc, Va = sets = [torch.full((K, ld // w), v, dtype=dt, device=DEV) for v, dt, w in zip(
        behind, (torch.float32, torch.float32, torch.uint8, torch.float32, torch.uint8, torch.float32),
        (1, 1, 1, 64, 1, 64))]
    P[:, :n], Mc[:, :n], Vc[:, :n], Ma[:, :b], Va[:, :b] = torch.from_numpy(p0).to(DEV), 127, 0, 0, 0
    coef = torch.tensor([clip, 1.0] * K, device=DEV) if clip else None
    want_p, state = [r.copy() for r in p0], [A.fresh(n) for _ in range(K)]
    for t in range(1, 4):
        g = np.stack([_row(rng, n, t) for _ in range(K)])
        G[:, :n] = torch.from_numpy(g).to(DEV)
        ops.adam8_step(P[:, :n], G[:, :n], Mc[:, :n], Ma[:, :b], Vc[:, :n], Va[:, :b], clip_coef=coef,
                       **adam_scalars(dict(HP, weight_decay=0.1, decoupled_weight_decay=decoupled), t))
        got = [x.cpu().numpy() for x in sets]
        for k in range(K):
            want_p[k], g_left, state[k] = A.step(want_p[k], g[k], state[k], t, weight_decay=0.1, decoupled=decoupled,
                                                 clip=clip, **HP)
            for name, have, want in zip(("param", "grad") + KEYS, got, (want_p[k], g_left) + state[k]):
                assert have[k, :len(want)].tobytes() == want.tobytes(), (t, k, name)
        assert t > 1 or (state[0][0][0], state[0][2][0], state[0][2][1]) == (0, 255, 1)  # -1, 1, the code-1 rule
    for x, keep, cut in zip(got, behind, (n, n, n, b, n, b)):
        assert (x[:, cut:] == keep).all()  # nothing behind n was touched


@pytest.mark.parametrize("clip", [None, 0.37], ids=["noclip", "clip"])
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "l2"])
@pytest.mark.parametrize("n,K", [(64, 1), (64, 3), (192, 1), (192, 3), (64 * 37, 1), (64 * 37, 3)])
def test_step_kernel_bit_for_bit(n, K, decoupled, clip):
    _check_step(n, K, decoupled, clip)


def test_step_kernel_second_trip_of_the_grid():
    _check_step(LONG, 1, True, 0.37)


@pytest.mark.parametrize("row", [0, 1], ids=["signed", "unsigned"])
def test_encode_kernel_bit_for_bit(row):
    from gym_amd import ops
    K, n = 3, 64 * 37
    rng = np.random.default_rng(row)
    x = np.stack([_row(rng, n, k) * rng.lognormal(0, 3, n).astype(np.float32) for k in range(K)])
    x[0, 192:256] = A.tables()[1][row, 100:164] * 2  # ties: on a threshold once divided by the block's absmax 2
    x[0, 192] = 2.0
    x = np.abs(x) if row else x
    X = torch.zeros(K, n + 64, device=DEV)
    X[:, :n] = torch.from_numpy(x).to(DEV)
    C = torch.full((K, n + 64), 99, dtype=torch.uint8, device=DEV)
    S = torch.full((K, n // 64 + 1), 3.0, device=DEV)
    ops.adam8_encode(X[:, :n], C[:, :n], S[:, :n // 64], row)
    for k in range(K):
        q, am = A.encode(x[k], row)
        assert np.array_equal(C[k, :n].cpu().numpy(), q) and np.array_equal(S[k, :n // 64].cpu().numpy(), am)
    assert bool((C[:, n:] == 99).all()) and bool((S[:, n // 64:] == 3.0).all())


def _build(replica, K):
    """(models, optimizer, step function, arena) of a DiLoCo strategy with the "adamw8bit" inner spec."""
    from tiny_models import TinyMLP
    from gym_amd.replica import ReplicaRunner
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    torch.manual_seed(3)
    models = [TinyMLP().to(DEV) for _ in range(K)]
    s = DiLoCoStrategy(optim_spec=OptimSpec.from_string("adamw8bit", weight_decay=0.1, **HP), H=100)
    if replica:
        runner = ReplicaRunner(s, models, rank=0, num_nodes=K)
        return models, runner.optim, runner.step, runner.ra
    s._init_node(models[0], 0, 1)
    return models, s.optim, s.step, s.arena


def _run(models, step, arena, steps, shadows=()):
    """Steps `steps` on seeded gradients, fc2.bias absent on steps 2 and 3; shadows: [(parameters, optimizers)] per model."""
    for t in steps:
        arena.zero_grad()
        for k, m in enumerate(models):
            gen = torch.Generator().manual_seed(1000 * t + k)
            for i, (name, p) in enumerate(m.named_parameters()):
                g = (torch.randn(p.shape, generator=gen) * 10.0 ** (i - 2)).to(DEV)
                gone = name == "fc2.bias" and t in (2, 3)
                if gone:
                    p.grad = None
                else:
                    p.grad.copy_(g)
                for ps, _ in shadows:
                    ps[k][i].grad = None if gone else g.clone()
        step()
        for _, opts in shadows:
            for o in opts:
                o.step()


@pytest.mark.parametrize("replica,K", [(False, 1), (True, 3)], ids=["process", "replica"])
def test_build_fused_matches_the_torch_class(replica, K):
    from gym_amd.fused_optim import ArenaAdam8bit
    from gym_amd.strategy.optim import AdamW8bit
    models, opt, step, arena = _build(replica, K)
    assert type(opt) is ArenaAdam8bit and opt.placement == {"placed": False, "why": "no search for 8-bit AdamW"}
    assert opt.state_bytes() <= 0.27 * 8 * opt.K * opt.ld
    clone = lambda: [[torch.nn.Parameter(p.detach().clone()) for p in m.parameters()] for m in models]  # noqa: E731
    p8, p32 = clone(), clone()
    shadows = [(p8, [AdamW8bit(ps, weight_decay=0.1, **HP) for ps in p8]),
               (p32, [torch.optim.AdamW(ps, weight_decay=0.1, **HP) for ps in p32])]
    bias = [m.fc2.bias for m in models]
    _run(models, step, arena, [0, 1], shadows)
    held = [(b.detach().clone(), {k: v.clone() for k, v in opt.state[b].items()}) for b in bias]
    _run(models, step, arena, [2, 3], shadows)
    for b, (value, st) in zip(bias, held):  # absent: value, codes, scales and count (2) stay
        assert torch.equal(b, value) and all(torch.equal(opt.state[b][k], st[k]) for k in st)
    _run(models, step, arena, [4, 5], shadows)
    assert float(opt.state[bias[0]]["step"]) == 4.0 and float(opt.state[models[0].fc1.weight]["step"]) == 6.0
    far = lambda xs, ys: max(float((p.detach() - q.detach()).abs().max()) for x, y in zip(xs, ys)  # noqa: E731
                             for p, q in zip(x, y))
    d, D = far([list(m.parameters()) for m in models], p8), far(p8, p32)
    print(f"adam8bit build_fused {'replica' if replica else 'process'} K={K}: d = {d:.3e} (fused against AdamW8bit), "
          f"D = {D:.3e} (AdamW8bit against fp32 AdamW)")
    assert D > 0 and d <= 0.1 * D
    assert d <= 4 * 0.0  # d_measured = 0 in both modes (profiles/inner_adam8bit.txt)
    for m, ps, o in zip(models, *shadows[0]):  # and the state has the torch class's layout and values
        for p, q in zip(m.parameters(), ps):
            assert all(torch.equal(opt.state[p][k], o.state[q][k]) for k in KEYS)


def test_resume_continues_bit_identically():
    """Three steps, state_dict() into a fresh ArenaAdam8bit, three more in both: the same bits.  Then a
    torch.optim.AdamW state dict loads through ga_adam8_encode."""
    models, opt, step, arena = _build(True, 3)
    _run(models, step, arena, range(3))
    models2, opt2, step2, arena2 = _build(True, 3)
    arena2.flat_set.copy_(arena.flat_set)
    opt2.load_state_dict(opt.state_dict())
    _run(models, step, arena, range(3, 6))
    _run(models2, step2, arena2, range(3, 6))
    assert torch.equal(arena.flat_set, arena2.flat_set)
    assert all(torch.equal(getattr(opt, x), getattr(opt2, x)) for x in ("_Mc", "_Ma", "_Vc", "_Va"))
    assert [float(opt2.state[p]["step"]) for p in models2[0].parameters()] == [6.0, 6.0, 6.0, 4.0]
    ps = [torch.nn.Parameter(p.detach().clone()) for m in models for p in m.parameters()]
    plain = torch.optim.AdamW(ps, **HP)
    for p in ps:
        p.grad = torch.randn_like(p)
    plain.step()
    opt2.load_state_dict(plain.state_dict())
    st, n = opt2.state[models2[0].fc1.weight], ps[0].numel()
    for key, row in (("exp_avg", 0), ("exp_avg_sq", 1)):
        code, am = A.encode(np.pad(plain.state[ps[0]][key].cpu().numpy().reshape(-1), (0, -n % 64)), row)
        assert np.array_equal(st[key + "_code"].cpu().numpy(), code)
        assert np.array_equal(st[key + "_absmax"].cpu().numpy(), am)
    assert float(st["step"]) == 1.0
