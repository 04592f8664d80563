"""oracle.optim.sgd_step pinned from both sides (CPU only): against torch.optim.SGD
(single-tensor, fp32, on the CPU) with the float64 bound of sgd_kernel_checks between
them, and against the CPU stand-in of the kernel (tests/fake_sgd_ops.py), which states
the same contract a second time and is what the CPU tests of ArenaSGD run on."""
import numpy as np
import pytest
import torch

import sgd_kernel_checks as C
from oracle import optim as ooptim

f32 = np.float32
N = 8343

TORCH_SETTINGS = {
    "plain": dict(momentum=0.0, dampening=0.0, nesterov=False),
    "momentum": dict(momentum=0.9, dampening=0.0, nesterov=False),
    "dampening": dict(momentum=0.9, dampening=0.9, nesterov=False),
    "nesterov": dict(momentum=0.9, dampening=0.0, nesterov=True),
}


@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("name", list(TORCH_SETTINGS))
def test_oracle_matches_torch_cpu_sgd_step_by_step(name, wd):
    """Four steps of torch.optim.SGD (the first one, then three ordinary ones); after
    each, the oracle run from torch's state before that step is within gamma_R * A of the
    float64 step and bit-identical to torch's p and momentum buffer in >= 0.999 of the
    elements.  Measured: 1.000000 for p and buf on every step of all eight settings."""
    kw = TORCH_SETTINGS[name]
    p0, _, _ = C.sgd_data(11, K=1, n=N)
    ref = torch.nn.Parameter(torch.from_numpy(p0[0].copy()))
    opt = torch.optim.SGD([ref], lr=C.LR, weight_decay=wd, foreach=False, **kw)
    mom = kw["momentum"] != 0
    for step in range(4):
        g = (np.random.default_rng(100 + step).standard_normal(N) * 0.05).astype(f32)
        p_before = ref.detach().numpy().copy()
        b_before = opt.state[ref]["momentum_buffer"].numpy().copy() if (mom and step) else None
        ref.grad = torch.from_numpy(g.copy())
        opt.step()
        v = C.variant(dict(kw, first=step == 0), wd)
        wp, wg, wb = ooptim.sgd_step(p_before, g, b_before, C.LR, weight_decay=wd, first=step == 0, **kw)
        ep, eb, a_p, a_b = C.sgd_exact(p_before, g, b_before, None, v)
        r_p, r_b = C.roundings(v, None)
        tag = f"oracle {name} wd {wd} step {step}"
        C.assert_within(wp, ep, a_p, r_p, tag + " p")
        share_p = float(C.same_bits(wp, ref.detach().numpy()).mean())
        share_b = None
        if mom:
            C.assert_within(wb, eb, a_b, r_b, tag + " buf")
            share_b = float(C.same_bits(wb, opt.state[ref]["momentum_buffer"].numpy()).mean())
        else:
            assert wb is None and opt.state[ref].get("momentum_buffer") is None
        print(f"{tag}: share bit-identical to torch p {share_p:.6f} buf {share_b}")
        assert share_p >= 0.999 and (share_b is None or share_b >= 0.999)
        assert C.same_bits(wg, g).all() and C.same_bits(ref.grad.numpy(), g).all()  # neither changes an unclipped g


def test_bound_counts_at_most_six_roundings_for_p_and_four_for_buf():
    worst = [C.roundings(C.variant(name, wd), coef) for name in C.FLAGS for wd in (0.0, 0.05) for coef in (None, 0.5)]
    assert max(r[0] for r in worst) == 6 and max(r[1] for r in worst) == 4
    assert C.roundings(C.variant("plain"), None) == (1, 0)
    assert C.roundings(C.variant("nesterov-first", 0.05), float("nan")) == (4, 2)


def test_oracle_first_step_and_no_momentum_ignore_the_buffer():
    p, g, b = (x[0] for x in C.sgd_data(12, K=1, n=257))
    nan = np.full_like(b, np.nan)
    for name in ("momentum-first", "dampening-first", "nesterov-first"):
        v = C.FLAGS[name]
        a = ooptim.sgd_step(p, g, b, C.LR, weight_decay=0.05, clip=0.5, **v)
        c = ooptim.sgd_step(p, g, nan, C.LR, weight_decay=0.05, clip=0.5, **v)
        assert all(C.same_bits(x, y).all() for x, y in zip(a, c)) and np.isfinite(a[0]).all()
    wp, wg, wb = ooptim.sgd_step(p, g, None, C.LR, weight_decay=0.05, clip=0.5)
    assert wb is None and C.same_bits(wg, (g * f32(0.5)).astype(f32)).all()
    assert C.same_bits(wp, ooptim.sgd_step(p, g, nan, C.LR, weight_decay=0.05, clip=0.5)[0]).all()


@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("name", list(C.FLAGS))
def test_stand_in_equals_oracle_bit_for_bit(name, wd, clipped):
    """fake_sgd_ops.sgd_step on [2, ld] sets with n < ld: p, the gradient left behind and
    buf equal the oracle's bit for bit per replica (clip_coef[2k] is replica k's), and the
    columns [n, ld) are not touched."""
    import fake_sgd_ops
    K, n, ld = 2, 1001, 1012
    v = C.variant(name, wd)
    mom = v["momentum"] != 0
    start = C.sgd_data(13, K=K, n=ld)
    P, G, B = (torch.from_numpy(x.copy()) for x in start)
    # replica 0's coefficient does not scale, replica 1's does; the norms between them are never read
    clip = torch.tensor([1.0, 7.0, 0.37, 9.0]) if clipped else None
    fake_sgd_ops.sgd_step(P, G, B if mom else None, clip_coef=clip, n=n, **C.launch_kw(v))
    for k in range(K):
        coef = float(clip[2 * k]) if clipped else None
        wp, wg, wb = ooptim.sgd_step(start[0][k, :n], start[1][k, :n], start[2][k, :n] if mom else None, v["lr"],
                                     v["momentum"], v["dampening"], wd, v["nesterov"], v["first"], clip=coef)
        assert C.same_bits(P[k, :n].numpy(), wp).all()
        assert C.same_bits(G[k, :n].numpy(), wg).all()
        assert C.same_bits(B[k, :n].numpy(), wb if mom else start[2][k, :n]).all()
        got = (P[k, :n].numpy(), G[k, :n].numpy(), B[k, :n].numpy() if mom else None)
        C.assert_sgd(got, (start[0][k, :n], start[1][k, :n], start[2][k, :n] if mom else None), coef, v,
                     f"stand-in {name} wd {wd} replica {k}")
    for T, x in zip((P, G, B), start):
        assert C.same_bits(T[:, n:].numpy(), x[:, n:]).all()


def test_stand_in_and_oracle_agree_on_a_nan_coefficient():
    import fake_sgd_ops
    p, g, b = C.sgd_data(14, K=1, n=64)
    P, G, B = (torch.from_numpy(x.copy()) for x in (p, g, b))
    v = C.variant("nesterov", 0.05)
    fake_sgd_ops.sgd_step(P, G, B, clip_coef=torch.tensor([float("nan"), float("nan")]), **C.launch_kw(v))
    wp, wg, wb = ooptim.sgd_step(p[0], g[0], b[0], v["lr"], 0.9, 0.0, 0.05, True, False, clip=float("nan"))
    for T, w in zip((P, G, B), (wp, wg, wb)):
        assert np.isnan(T.numpy()).all() and np.isnan(w).all()
