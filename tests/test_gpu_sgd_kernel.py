"""ga_sgd_step launched on its own (gym_amd.ops.sgd_step, no ArenaSGD around it):
every instantiation of SgdOp<kMomentum, kFirst, kNesterov> against the fp32 oracle
(oracle.optim.sgd_step) and the float64 bound of tests/sgd_kernel_checks.py, and the
geometry edges of opt_pass<Op> for SGD and Adam.

As in test_gpu_stream_kernels.py every buffer is longer than the kernel is told (row
stride ld > n, 64 elements behind the last row) and the rest holds a sentinel that
must be bit-unchanged after every launch.  One workgroup owns 1024 float4, so
n = 8343 is two full workgroups, a partial one and a 3-element scalar tail.
"""
import math

import numpy as np
import pytest
import torch

import optim_cases
import sgd_kernel_checks as C
from oracle import optim as ooptim
from sgd_kernel_checks import Placed, bits, host

pytestmark = pytest.mark.gpu

f32 = np.float32
N, LD = 8343, 8352


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gym_amd import _lib
    _lib.lib()


def place(start, ld, mom=True):
    """[P, G, B] for (p, g, buf) arrays ([K, n], or 1-D at ld None); B None without momentum."""
    p, g, b = start
    return [Placed(p, ld=ld), Placed(g, ld=ld), Placed(b, ld=ld) if mom else None]


def launch(sets, v, clip=None, n=None):
    from gym_amd import ops
    P, G, B = sets
    ops.sgd_step(P.view, G.view, B.view if B is not None else None, clip_coef=clip, n=P.n if n is None else n,
                 **C.launch_kw(v))


def clip_coefs(G, n, max_norm=1.0):
    """The [2K] device tensor of ga_grad_clip_coef over a placed gradient set."""
    from gym_amd import ops
    out = torch.zeros(2 * G.K, device=C.DEV)
    ops.grad_clip_coef(G.view, n, max_norm, ops.sumsq_partials(C.DEV, G.K), out)
    return out


def rows(x):
    return x.reshape(-1, x.shape[-1])


def state(sets):
    """(p, g, buf) as [K, n] host arrays (buf None when there is no buffer)."""
    return [rows(s.data()) if s is not None else None for s in sets]


def check_replicas(sets, start, coefs, v, tag, replicas=None):
    got, start = state(sets), [rows(np.asarray(x, f32)) if x is not None else None for x in start]
    mom = v["momentum"] != 0
    for k in (range(sets[0].K) if replicas is None else replicas):
        C.assert_sgd((got[0][k], got[1][k], got[2][k] if mom else None),
                     (start[0][k], start[1][k], start[2][k] if mom else None),
                     None if coefs is None else float(coefs[k]), v, f"{tag} replica {k}")
    assert all(s.outside_untouched() for s in sets if s is not None)


@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("name", list(C.FLAGS))
def test_sgd_step_every_variant_direct(name, wd, clipped):
    """[3, 8352] sets, n = 8343, per-replica coefficients from ga_grad_clip_coef (max_norm
    1: replica 0 is not clipped).  Measured on the MI355X: p and buf bit-identical to the
    oracle in a share of 1.000000 of the elements, every replica of all 28 cases."""
    v = C.variant(name, wd)
    mom = v["momentum"] != 0
    start = C.sgd_data(500 + list(C.FLAGS).index(name))
    sets = place(start, LD, mom)
    clip = coefs = None
    if clipped:
        clip = clip_coefs(sets[1], N)
        coefs = host(clip)[0::2]
        assert coefs[0] == 1.0 and coefs[1] < 1 and coefs[2] < 1
    launch(sets, v, clip)
    check_replicas(sets, start, coefs, v, f"sgd {name} wd {wd}")


@pytest.mark.parametrize("name", ["momentum-first", "dampening-first", "nesterov-first"])
def test_first_step_never_reads_the_buffer(name):
    """SgdOp<true, true, *>::kLoad is false: a buffer that holds NaN in [0, n) (and the
    sentinel elsewhere) gives finite parameters at the ordinary bars and leaves exactly
    the oracle's g (clipped, with weight decay, not dampened) in the buffer."""
    v = C.variant(name, 0.05)
    nesterov = v["nesterov"]
    start = list(C.sgd_data(510))
    start[2] = np.full_like(start[2], np.nan)
    sets = place(start, LD)
    assert np.isnan(sets[2].data()).all()
    clip = clip_coefs(sets[1], N)
    coefs = host(clip)[0::2]
    launch(sets, v, clip)
    got = state(sets)
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    check_replicas(sets, start, coefs, v, f"{name} over NaN")
    for k in range(3):  # the oracle's g: the step without dampening, whatever the variant's dampening
        _, _, wb = ooptim.sgd_step(start[0][k], start[1][k], None, v["lr"], 0.9, 0.0, 0.05, nesterov, True,
                                   clip=float(coefs[k]))
        assert C.same_bits(got[2][k], wb).all()


@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_no_momentum_never_touches_a_buffer(wd):
    """momentum = 0 has no state stream: a buffer passed anyway is bit-unchanged in every
    element, and the parameters equal those of the call with buf=None bit for bit."""
    v = C.variant("plain", wd)
    start = list(C.sgd_data(520))
    start[2] = np.full_like(start[2], C.SENT)
    with_buf, without = place(start, LD), place(start, LD, mom=False)
    clip = clip_coefs(with_buf[1], N)
    coefs = host(clip)[0::2]
    launch(with_buf, v, clip)
    launch(without, v, clip)
    assert with_buf[2].untouched()
    check_replicas(without, start, coefs, v, f"plain wd {wd} buf=None")
    check_replicas(with_buf[:2] + [None], start, coefs, v, f"plain wd {wd} buffer ignored")
    assert np.array_equal(with_buf[0].data_bits(), without[0].data_bits())
    assert np.array_equal(with_buf[1].data_bits(), without[1].data_bits())


EDGES = [1, 3, 4, 5, 4095, 4096, 4097, 4100, 8192]
EDGE_COEF = 0.37


@pytest.mark.parametrize("K", [1, 2], ids=["1d", "K2"])
@pytest.mark.parametrize("n", EDGES)
def test_opt_pass_geometry_edges(n, K):
    """opt_pass<SgdOp<true, false, true>> and opt_pass<AdamOp> where the work split
    changes: n < 4 (no vector, the tail alone in a grid of 1), one whole chunk without a
    tail (4096), a chunk and a tail in the only workgroup (4097), a second workgroup that
    owns one vector (4100), two whole chunks (8192); as 1-D buffers and as [2, ld] sets,
    the last replica clipped by a coefficient < 1."""
    from gym_amd import ops
    ld = None if K == 1 else (n + 3) // 4 * 4 + 8
    coefs = np.array([1.0] * (K - 1) + [EDGE_COEF], f32)
    clip = torch.zeros(2 * K, device=C.DEV)
    clip[0::2] = torch.from_numpy(coefs).to(C.DEV)

    def shaped(x):
        return x[0] if K == 1 else x

    v = C.variant("nesterov", 0.05)
    start = [shaped(x) for x in C.sgd_data(530 + n, K=K, n=n)]
    sets = place(start, ld)
    launch(sets, v, clip, n=n)
    check_replicas(sets, start, coefs, v, f"sgd edge n={n} K={K}")

    step, lr, betas, eps, wd = 4, 1e-3, (0.9, 0.999), 1e-8, 1e-2
    a_start = C.adam_data(540 + n, K=K, n=n)
    a_sets = [Placed(shaped(x), ld=ld) for x in a_start]
    ops.adam_step(*(s.view for s in a_sets), clip_coef=clip, n=n, **C.adam_hp(lr, betas, eps, wd, True, step))
    got = [rows(s.data()) for s in a_sets]
    kw = dict(lr=lr, betas=betas, eps=eps, weight_decay=wd, decoupled=True)
    for k in range(K):
        C.check_adam_replica([x[k] for x in got], [x[k] for x in a_start], float(coefs[k]), step, kw,
                              f"adamw edge n={n} K={K} replica {k}")
    assert all(s.outside_untouched() for s in a_sets)


def test_per_row_launches_equal_the_whole_set_launch():
    """ArenaSGD's partial-range form: three 1-D row launches, each with its own
    clip[2k:2k+2] slice, leave p, g and buf bit-identical to one [3, ld] launch."""
    v = C.variant("nesterov", 0.05)
    start = C.sgd_data(550)
    whole, by_row = place(start, LD), place(start, LD)
    clip = clip_coefs(whole[1], N)
    launch(whole, v, clip)
    from gym_amd import ops
    for k in range(3):
        P, G, B = (s.view[k] for s in by_row)
        ops.sgd_step(P, G, B, clip_coef=clip[2 * k:2 * k + 2], **C.launch_kw(v))
    for a, b in zip(whole, by_row):
        assert np.array_equal(a.data_bits(), b.data_bits())
        assert a.outside_untouched() and b.outside_untouched()
    check_replicas(whole, start, host(clip)[0::2], v, "whole-set launch")


def test_first_then_ordinary_step_chain():
    """A first launch, then an ordinary one on the state it left (Nesterov, weight decay,
    clipping): each step at the bars from the device's own state before it, the end within
    optim_cases.assert_close of torch.optim.SGD + clip_grad_norm_ on the CPU."""
    start = C.sgd_data(560)
    grads = [start[1], C.sgd_data(561)[1][::-1].copy()]  # step 2: the gradient scales reversed
    sets = place((start[0], grads[0], np.zeros_like(start[2])), LD)
    for step, first in enumerate((True, False)):
        v = C.variant("nesterov-first" if first else "nesterov", 0.05)
        if step:
            sets[1] = Placed(grads[step], ld=LD)
        before = state(sets)
        clip = clip_coefs(sets[1], N)
        launch(sets, v, clip)
        check_replicas(sets, before, host(clip)[0::2], v, f"chain step {step}")
    got = state(sets)
    for k in range(3):
        ref = torch.nn.Parameter(torch.from_numpy(start[0][k].copy()))
        opt = torch.optim.SGD([ref], lr=C.LR, momentum=0.9, nesterov=True, weight_decay=0.05, foreach=False)
        for g in grads:
            ref.grad = torch.from_numpy(g[k].copy())
            torch.nn.utils.clip_grad_norm_([ref], 1.0)
            opt.step()
        optim_cases.assert_close([got[0][k], got[2][k]],
                                 [ref.detach().numpy(), opt.state[ref]["momentum_buffer"].numpy()])
        np.testing.assert_allclose(got[1][k], ref.grad.numpy(), rtol=1e-5, atol=0)  # the clipped gradient


def _torch_sgd_step(p, g, b, max_norm):
    """(p, g, buf) of clip_grad_norm_ + torch.optim.SGD(momentum 0.9) on the CPU, from a given buffer."""
    ref = torch.nn.Parameter(torch.from_numpy(p.copy()))
    ref.grad = torch.from_numpy(g.copy())
    opt = torch.optim.SGD([ref], lr=C.LR, momentum=0.9, foreach=False)
    opt.state[ref]["momentum_buffer"] = torch.from_numpy(b.copy())
    if max_norm:
        torch.nn.utils.clip_grad_norm_([ref], max_norm)
    opt.step()
    return ref.detach().numpy(), ref.grad.numpy(), opt.state[ref]["momentum_buffer"].numpy()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_sgd_nonfinite_gradient_parity_with_torch(bad):
    """test_adam_nonfinite_gradient_parity_with_torch for SGD with momentum: one bad
    gradient element in replica 1.  Clipped, a NaN makes the replica's coefficient, whole
    gradient, buffer and parameters NaN, and +inf gives coefficient 0: zero gradients
    and one NaN, exactly where clip_grad_norm_ + torch.optim.SGD on the CPU put NaN.
    Unclipped, the bad element spoils only itself.  The neighbouring replicas and the
    other elements meet the ordinary bars."""
    at = 4321
    v = C.variant("momentum")
    start = C.sgd_data(570)
    start[1][1, at] = bad
    # clipped
    sets = place(start, LD)
    clip = clip_coefs(sets[1], N)
    launch(sets, v, clip)
    o = host(clip)
    got = state(sets)
    if math.isnan(bad):
        assert np.isnan(o[2]) and np.isnan(o[3])
    else:
        assert o[2] == 0.0 and np.isposinf(o[3])
    ref = _torch_sgd_step(start[0][1], start[1][1], start[2][1], 1.0)
    for name, x, r in zip(("p", "g", "buf"), got, ref):
        print(f"{name}: NaN on the device {int(np.isnan(x[1]).sum())}, in torch {int(np.isnan(r).sum())} of {N}")
        assert np.array_equal(np.isnan(x[1]), np.isnan(r))
        assert int(np.isnan(r).sum()) == (N if math.isnan(bad) else 1)
        optim_cases.assert_close([x[1]], [r])  # NaN where torch has NaN, finite elements within the tolerance
    if not math.isnan(bad):
        assert not got[1][1][np.arange(N) != at].any()  # coefficient 0: the other gradients are zero
    check_replicas(sets, start, o[0::2], v, f"clipped {bad}", replicas=(0, 2))
    # unclipped
    sets = place(start, LD)
    launch(sets, v, None)
    got = state(sets)
    ref = _torch_sgd_step(start[0][1], start[1][1], start[2][1], None)
    spoiled = np.arange(N) == at
    for name, x, r in zip(("p", "g", "buf"), got, ref):
        assert np.array_equal(~np.isfinite(x[1]), spoiled), name
        assert np.array_equal(np.isnan(x[1]), np.isnan(r)) and np.array_equal(np.isinf(x[1]), np.isinf(r))
        assert np.array_equal(x[1][spoiled], r[spoiled], equal_nan=True)
        optim_cases.assert_close([x[1][~spoiled]], [r[~spoiled]])
    assert np.array_equal(bits(sets[1].buf), sets[1].before)
    check_replicas(sets, start, None, v, f"unclipped {bad}", replicas=(0, 2))
    C.assert_sgd([x[1][~spoiled] for x in got], [x[1][~spoiled] for x in start], None, v, f"unclipped {bad} replica 1")


@pytest.mark.parametrize("K", [1, 2], ids=["1d", "K2"])
def test_adam_and_clip_refuse_n_beyond_the_row(K):
    """ops.adam_step and ops.grad_clip_coef refuse n < 0 and n > the row length on the
    host, as ops.sgd_step does (the C entry points do not compare ld with n at K = 1, so
    the kernel would stream past a 1-D buffer): every operand is bit-unchanged and a
    valid call still works afterwards."""
    from gym_amd import ops
    n, ld = 520, 528
    hp = C.adam_hp(1e-3, (0.9, 0.999), 1e-8, 1e-2, True, 4)
    start = C.adam_data(580, K=K, n=n)
    sets = [Placed(x[0] if K == 1 else x, ld=None if K == 1 else ld) for x in start]
    row = sets[0].view.shape[-1]  # the 1-D view runs on into the pad: n + 64
    part, out = ops.sumsq_partials(C.DEV, K), torch.full((2 * K,), C.SENT, device=C.DEV)
    for bad_n in (row + 1, row + 4096, -1):
        with pytest.raises(ValueError, match="ld < n"):
            ops.adam_step(*(s.view for s in sets), n=bad_n, **hp)
        with pytest.raises(ValueError, match="ld < n"):
            ops.grad_clip_coef(sets[1].view, bad_n, 1.0, part, out)
    assert all(s.untouched() for s in sets)
    assert np.array_equal(host(out), np.full(2 * K, C.SENT, f32))
    ops.grad_clip_coef(sets[1].view, n, 1.0, part, out)
    coefs = C.check_clip(out, rows(start[1]).astype(np.float64), 1.0)[0::2]
    ops.adam_step(*(s.view for s in sets), clip_coef=out, n=n, **hp)
    got = [rows(s.data()) for s in sets]
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=True)
    for k in range(K):
        C.check_adam_replica([x[k] for x in got], [x[k] for x in start], float(coefs[k]), 4, kw, f"valid call {k}")
    assert all(s.outside_untouched() for s in sets)
