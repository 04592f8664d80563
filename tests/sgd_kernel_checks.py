"""What one fused SGD step (ga_sgd_step, its CPU stand-in, oracle.optim.sgd_step) is
held to -- TEST INFRASTRUCTURE shared by tests/test_oracle_sgd.py (CPU) and
tests/test_gpu_sgd_kernel.py (MI355X).

A variant is a dict of torch.optim.SGD's hyperparameters plus `first` (the parameter's
first step: buf = g, no dampening, the buffer is not read).  `sgd_exact` evaluates the
step in float64 from the fp32 inputs and the fp32-rounded scalars, together with the
same expressions over absolute values (A); R counts the fp32 roundings of the fp32
evaluation.  Every fp32 evaluation in any order of the same operations then lies
within gamma_R * A of the exact value, gamma_R = R u / (1 - R u), u = 2^-24 (the
standard bound for R roundings), so bar (a) is no property of one implementation.

The second half holds what the GPU tests of the streaming kernels share (`Placed`,
`host`, `bits`, the Adam and clip bars), so that no test file imports another.
"""
import math

import numpy as np
import torch

from oracle import optim as ooptim

f32 = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -149  # one fp32 subnormal step

LR = 0.1
# the flag sets of SgdOp<kMomentum, kFirst, kNesterov>'s five instantiations; dampening shares the
# momentum ones, and on a first step it must not apply (buf = g, not (1 - dampening) * g)
FLAGS = {
    "plain": dict(momentum=0.0, dampening=0.0, nesterov=False, first=False),
    "momentum-first": dict(momentum=0.9, dampening=0.0, nesterov=False, first=True),
    "momentum": dict(momentum=0.9, dampening=0.0, nesterov=False, first=False),
    "dampening-first": dict(momentum=0.9, dampening=0.9, nesterov=False, first=True),
    "dampening": dict(momentum=0.9, dampening=0.9, nesterov=False, first=False),
    "nesterov-first": dict(momentum=0.9, dampening=0.0, nesterov=True, first=True),
    "nesterov": dict(momentum=0.9, dampening=0.0, nesterov=True, first=False),
}
GRAD_SCALES = (1e-3, 0.05, 0.5)  # norms ~ 0.09, 4.6, 46 at n = 8343: with max_norm 1 replica 0 is not clipped


def variant(flags, weight_decay=0.0, lr=LR):
    return dict(FLAGS[flags] if isinstance(flags, str) else flags, lr=lr, weight_decay=weight_decay)


def launch_kw(v):
    """ops.sgd_step's keywords for a variant, as ArenaSGD._prepare computes them."""
    return dict(neg_lr=-float(v["lr"]), momentum=float(v["momentum"]), one_m_dampening=1 - float(v["dampening"]),
                weight_decay=float(v["weight_decay"]), nesterov=bool(v["nesterov"]), first=bool(v["first"]))


def sgd_data(seed, K=3, n=8343):
    """(p, g, buf) [K, n]: the magnitudes of adam_data below."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((K, n)) * 0.02).astype(f32)
    g = (rng.standard_normal((K, n)) * np.array(GRAD_SCALES[:K], f32)[:, None]).astype(f32)
    buf = (rng.standard_normal((K, n)) * 0.01).astype(f32)
    return p, g, buf


def scales(coef):
    return coef is not None and not coef >= 1.0  # a NaN coefficient scales too


def roundings(v, coef):
    """(R_p, R_buf): the fp32 roundings behind p and buf -- the clip product, the weight
    decay fma, buf*momentum and its fma (later steps), Nesterov's fma, the parameter's fma."""
    r_g = int(scales(coef)) + int(v["weight_decay"] != 0)
    if v["momentum"] == 0:
        return r_g + 1, 0
    r_buf = r_g + (0 if v["first"] else 2)
    return r_buf + int(v["nesterov"]) + 1, r_buf


def sgd_exact(p, g, buf, coef, v):
    """(p, buf, A_p, A_buf) of the step in float64; buf and A_buf are None without momentum."""
    d = np.float64
    p, g = np.asarray(p, f32).astype(d), np.asarray(g, f32).astype(d)
    lr, mu = d(f32(-float(v["lr"]))), d(f32(v["momentum"]))
    omd, wd = d(f32(1 - float(v["dampening"]))), d(f32(v["weight_decay"]))
    a_g = np.abs(g)
    if scales(coef):
        c = d(f32(coef))
        g, a_g = g * c, a_g * abs(c)
    if wd != 0:
        g, a_g = g + wd * p, a_g + abs(wd) * np.abs(p)
    nb = a_b = None
    if mu != 0:
        if v["first"]:
            nb, a_b = g, a_g
        else:
            b = np.asarray(buf, f32).astype(d)
            nb, a_b = mu * b + omd * g, abs(mu) * np.abs(b) + abs(omd) * a_g
        if v["nesterov"]:
            g, a_g = g + mu * nb, a_g + abs(mu) * a_b
        else:
            g, a_g = nb, a_b
    return p + lr * g, nb, np.abs(p) + abs(lr) * a_g, a_b


def gamma(R):
    return R * U / (1 - R * U)


def assert_within(got, exact, A, R, what):
    """Bar (a): |got - exact| <= gamma_R * A + 2^-149, element by element."""
    err = np.abs(np.asarray(got, f32).astype(np.float64) - exact)
    bound = gamma(R) * A + TINY
    worst = float(np.max(err / np.maximum(A, TINY))) / U
    print(f"{what}: worst error {worst:.3f} u*A against gamma_{R} = {gamma(R) / U:.3f} u")
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (what, bad[:8], np.asarray(got)[bad[:8]], exact[bad[:8]])


def same_bits(a, b):
    return np.asarray(a, f32).view(np.int32) == np.asarray(b, f32).view(np.int32)


def assert_sgd(got, start, coef, v, tag):
    """One replica of one step.  got = (p, g, buf) after it, start = (p, g, buf) before
    (buf None without momentum), coef the clip coefficient that applied (None or >= 1:
    not clipped).
    (a) p and buf within gamma_R * A + 2^-149 of sgd_exact;
    (b) p and buf bit-identical to oracle.optim.sgd_step in a share >= 0.999 each;
    (c) the gradient left behind bit-equal to fl(g * coef) when clipped, bit-unchanged
        otherwise (never g + wd*p, never Nesterov's g).
    Returns the two shares (buf's None without momentum)."""
    p0, g0, b0 = start
    gp, gg, gb = got
    mom = v["momentum"] != 0
    ep, eb, a_p, a_b = sgd_exact(p0, g0, b0, coef, v)
    r_p, r_b = roundings(v, coef)
    assert_within(gp, ep, a_p, r_p, f"{tag} p")
    if mom:
        assert_within(gb, eb, a_b, r_b, f"{tag} buf")
    wp, wg, wb = ooptim.sgd_step(p0, g0, b0, v["lr"], v["momentum"], v["dampening"], v["weight_decay"], v["nesterov"],
                                 v["first"], clip=coef)
    share_p = float(same_bits(gp, wp).mean())
    share_b = float(same_bits(gb, wb).mean()) if mom else None
    print(f"{tag}: coef {coef!r}; bit-identical share p {share_p:.6f} buf "
          + (f"{share_b:.6f}" if mom else "none"))
    assert share_p >= 0.999, (tag, "p", share_p)
    assert not mom or share_b >= 0.999, (tag, "buf", share_b)
    with np.errstate(over="ignore", invalid="ignore"):
        left = (np.asarray(g0, f32) * f32(coef)).astype(f32) if scales(coef) else np.asarray(g0, f32)
    assert same_bits(left, wg).all()  # the oracle's own g_left is this value
    assert same_bits(gg, left).all(), (tag, "the gradient left behind", np.flatnonzero(~same_bits(gg, left))[:8])
    return share_p, share_b


# ---------------------------------------------------------------- placement ---
# What the GPU tests of the streaming kernels share (tests/test_gpu_stream_kernels.py,
# tests/test_gpu_sgd_kernel.py): buffers placed inside sentinel-filled allocations and
# the bars of the Adam and clip kernels.
DEV = "cuda:0"
SENT = -7.25  # exact in fp32 and bf16


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


def host(x):
    torch.cuda.synchronize()
    return x.float().cpu().numpy()


def bits(x):
    """The tensor's bit patterns on the host (int32 for fp32, int16 for bf16)."""
    torch.cuda.synchronize()
    return x.contiguous().view(torch.int32 if x.element_size() == 4 else torch.int16).cpu().numpy()


class Placed:
    """`data` ([n] or [K, n], fp32 values) inside a longer sentinel-filled allocation:
    `off` sentinel elements, K rows of stride ld >= n, `pad` sentinel elements.
    .view is what the kernel gets: the [K, n] rows (stride ld), or for 1-D data the
    buffer from `off` on (n elements and the pad behind them)."""

    def __init__(self, data, ld=None, off=0, pad=64, dtype=torch.float32):
        a = np.asarray(data, f32)
        rows = a.reshape(-1, a.shape[-1])
        self.K, self.n = rows.shape
        ld = self.n if ld is None else ld
        assert ld >= self.n
        self.buf = torch.full((off + self.K * ld + pad,), SENT, dtype=dtype, device=DEV)
        body = self.buf[off:off + self.K * ld].view(self.K, ld)
        body[:, :self.n] = t(rows, dtype)
        self.rows = body[:, :self.n]
        self.view = self.rows if a.ndim == 2 else self.buf[off:]
        self.inside = np.zeros(self.buf.numel(), bool)
        for k in range(self.K):
            self.inside[off + k * ld:off + k * ld + self.n] = True
        self.one_d = a.ndim == 1
        self.before = bits(self.buf)

    def data(self):
        x = host(self.rows).copy()
        return x[0] if self.one_d else x

    def data_bits(self):
        x = bits(self.rows)
        return x[0] if self.one_d else x

    def outside_untouched(self):
        b = bits(self.buf)
        return np.array_equal(b[~self.inside], self.before[~self.inside])

    def untouched(self):
        return np.array_equal(bits(self.buf), self.before)


def check_clip(out, rows_f64, max_norm):
    """The bars of test_gpu_optim.test_clip_coef_kernel against the float64 norm."""
    out = host(out)
    for k, row in enumerate(rows_f64):
        ref = math.sqrt(float(np.sum(row * row)))
        coef = min(1.0, max_norm / (ref + 1e-6))
        print(f"clip replica {k}: norm {out[2 * k + 1]!r} vs {ref!r}, coef {out[2 * k]!r} vs {coef!r}")
        assert abs(out[2 * k + 1] - ref) <= 1e-5 * ref
        assert abs(out[2 * k] - coef) <= 1e-5
    return out


N_ADAM, LD_ADAM = 8343, 8352  # 2085 float4 = two workgroups + a partial one, and a 3-element tail
ADAM_SCALES = (1e-3, 0.05, 0.5)  # gradient norms ~ 0.09, 4.6, 46 against max_norm 1: replica 0 is not clipped


def adam_hp(lr, betas, eps, wd, decoupled, step):
    """The launch parameters as ArenaAdam.step computes them."""
    b1, b2 = betas
    return dict(lerp_w=1 - b1, beta2=b2, one_m_beta2=1 - b2, eps=eps,
                wd_factor=(1 - lr * wd) if (decoupled and wd != 0) else 1.0,
                l2_wd=wd if (not decoupled and wd != 0) else 0.0, step_size=-(lr / (1 - b1 ** step)),
                bc2_sqrt=math.sqrt(1 - b2 ** step))


def adam_data(seed, K=3, n=N_ADAM, zero_state=False):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((K, n)) * 0.02).astype(f32)
    g = (rng.standard_normal((K, n)) * np.array(ADAM_SCALES[:K], f32)[:, None]).astype(f32)
    m = (rng.standard_normal((K, n)) * 0.01).astype(f32)
    v = (rng.random((K, n)) * 1e-4 + 1e-8).astype(f32)
    if zero_state:
        m[:], v[:] = 0, 0
    return p, g, m, v


def check_adam_replica(got, start, coef, step, kw, tag):
    """One replica of a fused step against oracle.optim.adam_step fed the coefficient the
    device wrote: p at rtol 1e-5 / atol 1e-7, m and v at rtol 1e-6, the gradient left
    behind bit-equal to fp32(g * coef) when clipped and bit-unchanged otherwise."""
    p0, g0, m0, v0 = start
    gp, gg, gm, gv = got
    wp, _, wm, wv = ooptim.adam_step(p0, g0, m0, v0, step, clip=coef, **kw)
    print(f"{tag}: coef {coef!r}; bit-identical share p {(gp == wp).mean():.6f} m {(gm == wm).mean():.6f} "
          f"v {(gv == wv).mean():.6f}")
    np.testing.assert_allclose(gp, wp, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(gm, wm, rtol=1e-6, atol=0)
    np.testing.assert_allclose(gv, wv, rtol=1e-6, atol=0)
    left = (g0 * f32(coef)).astype(f32) if coef < 1.0 else g0
    assert np.array_equal(gg.view(np.int32), left.view(np.int32))
