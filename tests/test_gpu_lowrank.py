"""ga_lowrank_project / _orthonormalize / _backproject and ga_diloco_outer_lowrank on the
MI355X against tests/lowrank_checks.py (whole engine steps: test_gpu_outer_lowrank.py).  One arena holds a
row-band remainder with n % 4 != 0 and unaligned rows (33, 70), whole bands (64, 256), three
bands and a short last tile (96, 520), more tiles than waves (32, 4100), a 4-D tensor, and
two tensors that never compress."""
import numpy as np
import pytest
import torch

import lowrank_checks as C
from sgd_kernel_checks import DEV

pytestmark = pytest.mark.gpu
f32, U = np.float32, C.U
SHAPES = [(33, 70), (64, 256), (96, 520), (32, 4100), (40, 3, 3, 3), (5,), (1, 300)]
HP = dict(lr=0.7, momentum=0.9, nesterov=True, dampening=0.0, weight_decay=1e-3)
PLAIN = dict(lr=1.0, momentum=0.0, nesterov=False, dampening=0.0, weight_decay=0.0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_plan(rank, shapes=SHAPES):
    from gym_amd.arena import ArenaLayout
    from gym_amd.lowrank import LowRankPlan
    L = ArenaLayout(shapes)
    return LowRankPlan(L.shapes, L.offsets, L.n, rank).to(DEV), L


def arena(L, rng, scale, rows=None):
    """Gaussian values on the tensors, 0 on the padding."""
    out = np.zeros((rows or 1, L.n), f32)
    for o, n in zip(L.offsets, L.numels):
        out[:, o:o + n] = scale * rng.standard_normal((out.shape[0], n))
    return out if rows else out[0]


def data(L, K, feedback, seed=0):
    rng = np.random.default_rng(seed)
    master = arena(L, rng, 1.0)
    X = (master + arena(L, rng, 1e-2, K)).astype(f32)
    return master, X, arena(L, rng, 1e-3, K) if feedback else None, arena(L, rng, 1e-3)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def chain(length, back):
    from gym_amd import ops
    return ops.lowrank_chain(length, back)


def same(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.int32), np.asarray(b, f32).view(np.int32))


def run_outer(plan, A, B, K, master, X, E, mom, hp, first):
    from gym_amd import ops
    tm, tx, te, tb = dev(master), dev(X), dev(E), dev(mom if hp["momentum"] else None)
    ops.diloco_outer_lowrank(plan, dev(A), dev(B), float(K), tx, te, tm, tb, K, hp["lr"], hp["momentum"],
                             hp["dampening"], hp["weight_decay"], hp["nesterov"], first)
    return tm.cpu().numpy(), None if tb is None else tb.cpu().numpy(), tx.cpu().numpy(), None if te is None else te.cpu().numpy()


@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("rank", [4, 32])
def test_kernels_against_the_oracle_phase_by_phase(rank, K, feedback):
    from gym_amd import ops
    plan, L = make_plan(rank)
    assert len(plan.compressed) >= 2 and len(SHAPES) - len(plan.compressed) >= 2
    master, X, E, mom = data(L, K, feedback, seed=rank + K)
    Q = plan.warm_start(3).numpy()
    tm, tx, te = dev(master), dev(X), dev(E)
    # project
    A = torch.full((plan.a_len,), 7.0, device=DEV)
    ops.lowrank_project(plan, tx, tm, te, dev(Q), 1.0, A)
    A, A64 = A.cpu().numpy(), C.project(plan, master, X, E, Q)
    bound = C.product_bound(plan, master, X, E, Q, chain, K, False)
    for t, P in C.views(plan, A, "p").items():
        err = np.abs(P - C.views(plan, A64, "p")[t])
        print(f"project r={rank} K={K} tensor {t}: max err/bound {(err / bound[t]).max():.2e}")
        assert (err <= bound[t]).all(), t
    sums = C.project(plan, master, X, None, Q, f32)
    for off, ln, aoff in plan.segments:
        assert same(A[aoff:aoff + ln], sums[aoff:aoff + ln])
    # back-project, from the oracle's orthonormal factors
    Ah = C.orthonormalize_all(plan, A64).astype(f32)
    Ah[plan.p_len:] = sums[plan.p_len:]  # the dense slots as the project launch leaves them
    B = torch.full((plan.b_len,), 7.0, device=DEV)
    ops.lowrank_backproject(plan, tx, tm, te, dev(Ah), B)
    B, B64 = B.cpu().numpy(), C.backproject(plan, master, X, E, Ah)
    bound = C.product_bound(plan, master, X, E, Ah, chain, K, True)
    for t, Bt in C.views(plan, B, "q").items():
        err = np.abs(Bt - C.views(plan, B64, "q")[t])
        print(f"back-project r={rank} K={K} tensor {t}: max err/bound {(err / bound[t]).max():.2e}")
        assert (err <= bound[t]).all(), t
    # decode: g alone (zero master, lr 1: the new master is -g exactly), then the whole update
    Bh = B64.astype(f32)
    g64, E64, m64, b64 = C.outer(plan, Ah, Bh, K, master, X, E, mom, HP, False)
    gb = C.g_bound(plan, Ah, Bh, K)
    comp = gb > 0
    zero = np.zeros_like(master)
    g0 = C.outer(plan, Ah, Bh, K, zero, X, None, None, PLAIN, True)[0]
    got = -run_outer(plan, Ah, Bh, K, zero, X, None, None, PLAIN, True)[0]
    assert (np.abs(got - g0)[comp] <= gb[comp]).all() and np.array_equal(g0[comp], g64[comp])
    gm, gmom, gx, ge = run_outer(plan, Ah, Bh, K, master, X, E, mom, HP, False)
    mb, bb = C.update_bounds(gb, g64, master, mom, HP, False)
    assert (np.abs(gm - m64)[comp] <= mb[comp]).all() and (np.abs(gmom - b64)[comp] <= bb[comp]).all()
    assert all(same(row, gm) for row in gx)
    if feedback:
        S = np.abs(master) + np.abs(X) + np.abs(E)
        assert (np.abs(ge - E64)[:, comp] <= (gb + 4 * U * S)[:, comp]).all() and same(ge[:, ~comp], E[:, ~comp])
    # dense elements and padding: ga_diloco_outer's bits
    dm, db, dx = dev(master), dev(mom), dev(X)
    ops.diloco_outer(dx, dm, db, dx, L.n, float(K), HP["lr"], HP["momentum"], HP["dampening"], HP["weight_decay"],
                     HP["nesterov"], False)
    dense = np.zeros(L.n, bool)
    for off, ln, _ in plan.segments:
        dense[off:off + ln] = True
    assert same(gm[dense], dm.cpu().numpy()[dense]) and same(gmom[dense], db.cpu().numpy()[dense])
    pad = np.ones(L.n, bool)
    for o, n in zip(L.offsets, L.numels):
        pad[o:o + n] = False
    assert not gm[pad].any() and not gx[:, pad].any() and not gmom[pad].any()


def orth_on_gpu(P):
    """ga_lowrank_orthonormalize on one m x r factor: a one-tensor plan whose matrix is m x 4096."""
    from gym_amd import ops
    from gym_amd.lowrank import LowRankPlan
    m, r = P.shape
    plan = LowRankPlan([(m, 4096)], [0], m * 4096, r).to(DEV)
    assert plan.compressed == [0] and plan.a_len == -(-m * r // 4) * 4
    A = torch.zeros(plan.a_len, device=DEV)
    A[:m * r] = dev(P.reshape(-1))
    ops.lowrank_orthonormalize(plan, A)
    return A.cpu().numpy()[:m * r].reshape(m, r)


@pytest.mark.parametrize("m,r", [(33, 1), (1000, 4), (1000, 32)])
def test_orthonormalize_gaussian(m, r):
    P = np.random.default_rng(m + r).standard_normal((m, r)).astype(f32)
    ref, got = C.orthonormalize(P), orth_on_gpu(P)
    own = np.abs(C.orthonormalize(P, f32) - ref).max()
    print(f"orthonormalize m={m} r={r}: kernel deviation / float32 restatement's {np.abs(got - ref).max() / own:.2f}")
    # tree reductions against numpy's pairwise sums: another order, the same error class
    # (measured ratios 2.11, 1.08 and 5.11)
    assert np.abs(got - ref).max() <= 8 * own


def test_orthonormalize_zero_and_rank_deficient():
    """An all-zero P gives exact zeros, nothing non-finite.  A rank-2 P at r = 4 (small
    integers: exactly rank 2 in fp32) gives exactly two zero columns and two orthonormal
    ones that span P; tolerance 8 m U, the worst case of an m-term fp32 dot product."""
    assert not orth_on_gpu(np.zeros((200, 4), f32)).any()
    rng = np.random.default_rng(2)
    m = 200
    P = (rng.integers(-8, 9, (m, 2)) @ rng.integers(-4, 5, (2, 4))).astype(f32)
    got = orth_on_gpu(P).astype(np.float64)
    G, tol = got.T @ got, 8 * m * U
    assert np.isfinite(got).all() and ((got == 0).all(axis=0)).sum() == 2
    assert np.abs(G - np.diag(np.diag(G))).max() <= tol and (np.abs(np.diag(G)[np.diag(G) > 0] - 1) <= tol).all()
    assert np.abs(got @ (got.T @ P) - P).max() <= tol * np.abs(P).max()
