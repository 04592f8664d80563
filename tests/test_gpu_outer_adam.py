"""ga_diloco_outer_adam / ga_diloco_outer_adam_masked on the MI355X: every path
of the kernel (vector, scalar by length, scalar by alignment; K below, at and
across the unroll by 8; in place, one row to a separate row, K rows to one) for
f32 and bf16 arenas against the oracle (oracle.reduce.mean_reduce, an fp32
subtract, oracle.optim.adam_step), ONE step from a shared pre-state each (see
tests/outer_adam_checks.py for why never a trajectory), the masked form against
the two launches it replaces, the engine's step count over three device steps,
and the argument errors.

Measured on the MI355X (printed by the tests, not asserted): master, exp_avg and
exp_avg_sq bit-identical to the oracle in a share of 1.000000 of the elements in
every case of test_one_step_against_the_oracle (432 launches) and in the three
engine steps.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import outer_adam_checks as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
LD = 8352
N_VEC = 2 * 4096 + 4 * 37  # 8340: 2085 vectors = two full workgroups + 37 vectors
N_SCALAR = 8343            # odd: the whole launch takes the scalar kernel
GUARD = 64
SENT = -7.25               # exact in fp32 and bf16
ZERO = (np.arange(64) * 131 + 5) % N_VEC  # 64 elements spread over the three workgroups: every row == master

LAYOUTS = {"vector": (N_VEC, 0), "scalar-n": (N_SCALAR, 0), "scalar-offset": (N_VEC, 1)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gym_amd import _lib
    _lib.lib()


@pytest.fixture(autouse=True)
def _real_kernel_layer(monkeypatch):
    """These tests run the product's kernels: a CPU stand-in that an earlier test of
    the same process left installed in the gym_amd modules is put aside for them."""
    import sys

    import gym_amd.ops as real
    import gym_amd.replica  # noqa: F401  (imports every module that binds `ops`)
    import gym_amd.strategy  # noqa: F401
    for name, mod in list(sys.modules.items()):
        if name.startswith("gym_amd") and getattr(mod, "ops", real) is not real:
            monkeypatch.setattr(mod, "ops", real)


def bits(x):
    torch.cuda.synchronize()
    return x.contiguous().view(torch.int32 if x.element_size() == 4 else torch.int16).cpu().numpy()


class Buf:
    """K rows of stride LD inside a sentinel-filled allocation: `off` sentinel
    elements, the rows (data in columns [0, n), sentinels in [n, LD)), GUARD
    sentinel elements.  .rows is the [K, LD] view a kernel gets."""

    def __init__(self, data, dtype=torch.float32, off=0):
        a = np.asarray(data, f32)
        a = a.reshape(-1, a.shape[-1])
        self.K, self.n = a.shape
        self.buf = torch.full((off + self.K * LD + GUARD,), SENT, dtype=dtype, device=DEV)
        self.rows = self.buf[off:off + self.K * LD].view(self.K, LD)
        self.rows[:, :self.n] = torch.from_numpy(a).to(DEV, dtype)
        self.inside = np.zeros(self.buf.numel(), bool)
        for k in range(self.K):
            self.inside[off + k * LD:off + k * LD + self.n] = True
        self.before = bits(self.buf)

    def values(self):
        """The data columns widened to fp32 on the host."""
        torch.cuda.synchronize()
        return self.rows[:, :self.n].float().cpu().numpy()

    def assert_outside_unchanged(self, what):
        now = bits(self.buf)
        assert np.array_equal(now[~self.inside], self.before[~self.inside]), f"{what}: wrote outside its rows"

    def assert_unchanged(self, what):
        assert np.array_equal(bits(self.buf), self.before), f"{what} changed"


def make_state(seed, n, t):
    """(master, exp_avg, exp_avg_sq) fp32 of LD elements each; zero moments at t == 1.
    The ZERO elements of the master are bf16 values, so K equal rows sum and
    divide exactly and the pseudo-gradient there is exactly 0 for every K."""
    rng = np.random.default_rng(seed)
    master = (rng.standard_normal(LD) * 0.02).astype(f32)
    master[ZERO] = torch.from_numpy(master[ZERO]).bfloat16().float().numpy()
    if t == 1:
        m, v = np.zeros(LD, f32), np.zeros(LD, f32)
    else:
        m = (rng.standard_normal(LD) * 1e-3).astype(f32)
        v = (rng.random(LD) * 1e-6 + 1e-10).astype(f32)
    return master, m, v


def make_rows(seed, K, n, master):
    rng = np.random.default_rng(seed + 1000)
    rows = (master[:n] + rng.standard_normal((K, n)) * 1e-3).astype(f32)
    rows[:, ZERO] = master[ZERO]
    return rows


def hp_of(decay, betas, lr=0.05):
    wd, decoupled = {"none": (0.0, False), "adam-l2": (0.05, False), "adamw": (0.01, True)}[decay]
    return dict(lr=lr, betas=betas, eps=1e-8, weight_decay=wd, decoupled=decoupled)


def scalars(hp, t):
    from gym_amd.engine import DiLoCoOuterAdam

    class Local:
        world, rank, exchange, rccl, backend = 1, 0, False, False, "none"
    eng = DiLoCoOuterAdam(Local(), 1, 4, "cpu", torch.float32, **hp)
    return eng.scalars(t)


def run_form(dtype, K, layout, form, t, betas, decay, seed):
    from gym_amd import ops
    n, off = LAYOUTS[layout]
    hp = hp_of(decay, betas)
    master, m, v = make_state(seed, n, t)
    src = Buf(make_rows(seed, K, n, master), dtype, off)
    st = [Buf(x[None, :], torch.float32) for x in (master, m, v)]  # LD elements each: state beyond n is data
    for s in st:  # ...that the step must leave alone
        s.inside[:] = False
        s.inside[:n] = True
    dst = src if form == "inplace" else Buf(np.zeros((1, n), f32), dtype, off)
    rows0 = src.values()
    ops.diloco_outer_adam(src.rows[:, :n], st[0].rows[0], st[1].rows[0], st[2].rows[0], dst.rows[:, :n], n, K,
                          **scalars(hp, t))
    got = [s.values()[0][:n] for s in st]
    want = C.oracle_step(rows0, K, master[:n], m[:n], v[:n], t, hp)
    tag = f"{dtype} K={K} {layout} {form} t={t} betas={betas} {decay}"
    shares = C.bit_shares(got, want)
    C.assert_step(got, want, tag)
    assert all(np.isfinite(x).all() for x in got), tag
    if t == 1 and decay == "none":  # g == 0 with zero moments: 0 / eps, the master stays
        assert np.array_equal(got[0][ZERO].view(np.int32), master[ZERO].view(np.int32)), tag
        assert not got[1][ZERO].any() and not got[2][ZERO].any(), tag
    out = st[0].rows[0, :n].to(dtype)  # every output row is the master cast to the arena dtype, bitwise
    for j in range(dst.K):
        assert np.array_equal(bits(dst.rows[j, :n]), bits(out)), f"{tag}: row {j}"
    for b in st + [src, dst]:
        b.assert_outside_unchanged(tag)
    if dst is not src:
        src.assert_unchanged(f"{tag}: src")
    return shares


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("K", [1, 3, 9])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_one_step_against_the_oracle(dtype, K, layout):
    forms = ["inplace", "shard" if K == 1 else "kout1"]  # one row to a separate row is the sharded branch's shape
    worst = [1.0, 1.0, 1.0]
    for i, (form, t, betas, decay) in enumerate(itertools.product(forms, (1, 4), ((0.9, 0.999), (0.3, 0.9)),
                                                                  ("none", "adam-l2", "adamw"))):
        shares = run_form(dtype, K, layout, form, t, betas, decay, seed=100 * K + i)
        worst = [min(a, b) for a, b in zip(worst, shares)]
    print(f"K={K} {layout}: lowest bit-identical share over 24 launches: master {worst[0]:.6f} "
          f"exp_avg {worst[1]:.6f} exp_avg_sq {worst[2]:.6f}")


def packed_mask(n, seed):
    """p = 0.1 bytes with one all-ones and one all-zero word, and their packed words."""
    from gym_amd import ops
    rng = np.random.default_rng(seed)
    mask = (rng.random(n) < 0.1).astype(np.uint8)
    mask[5 * 64:6 * 64] = 1
    mask[7 * 64:8 * 64] = 0
    words = torch.zeros(ops.sparta_mask_words(n), dtype=torch.int64, device=DEV)
    ops.sparta_pack_mask(torch.from_numpy(mask).to(DEV), n, words)
    return mask, words


@pytest.mark.parametrize("n", [N_VEC, N_SCALAR], ids=["vector", "scalar"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_masked_step_equals_the_two_launches(dtype, n):
    from gym_amd import ops
    K, t = 3, 4
    hp = hp_of("adamw", (0.9, 0.999))
    sc = scalars(hp, t)
    master, m, v = make_state(7, n, t)
    rows = make_rows(7, K, n, master)
    mask, words = packed_mask(n, 11)
    assert 0.05 < mask.mean() < 0.2
    two = [Buf(rows, dtype)] + [Buf(x[None, :], torch.float32) for x in (master, m, v)]
    one = [Buf(rows, dtype)] + [Buf(x[None, :], torch.float32) for x in (master, m, v)]
    ops.sparta_average_local(two[0].rows[:, :n], n, float(K), mask=words)
    ops.diloco_outer_adam(two[0].rows[:, :n], two[1].rows[0], two[2].rows[0], two[3].rows[0], two[0].rows[:, :n], n,
                          K, **sc)
    ops.diloco_outer_adam_masked(one[0].rows[:, :n], words, one[1].rows[0], one[2].rows[0], one[3].rows[0], n,
                                 float(K), K, **sc)
    for a, b, what in zip(one, two, ("rows", "master", "exp_avg", "exp_avg_sq")):
        assert np.array_equal(bits(a.buf), bits(b.buf)), what
    assert not np.array_equal(bits(one[1].buf), one[1].before)
    # ...and against the plain step only selected elements differ (the mask is not inert on a bf16 set)
    plain = [Buf(rows, dtype)] + [Buf(x[None, :], torch.float32) for x in (master, m, v)]
    ops.diloco_outer_adam(plain[0].rows[:, :n], plain[1].rows[0], plain[2].rows[0], plain[3].rows[0],
                          plain[0].rows[:, :n], n, K, **sc)
    diff = bits(plain[2].buf)[:n] != bits(one[2].buf)[:n]
    assert not diff[mask[:n] == 0].any()
    if dtype == torch.bfloat16:  # (an fp32 set at K = 3 averages back to the same sum: fl(fl(3a) / 3) == a)
        assert diff.any()


def _c(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def test_masked_step_refuses_a_call_that_is_not_in_place():
    from gym_amd import _lib
    L = _lib.lib()
    n, K = N_VEC, 3
    master, m, v = make_state(3, n, 4)
    bufs = [Buf(make_rows(3, K, n, master)), Buf(np.zeros((K, n), f32))] + [Buf(x[None, :]) for x in (master, m, v)]
    _, words = packed_mask(n, 5)
    sc = [float(x) for x in scalars(hp_of("none", (0.9, 0.999)), 4).values()]
    src, dst, pm, mm, vm = bufs
    rc = L.ga_diloco_outer_adam_masked(0, _c(src.rows), K, LD, n, _c(words), float(K), float(K), _c(pm.rows),
                                       _c(mm.rows), _c(vm.rows), *sc, _c(dst.rows), K, LD, None)
    assert rc == 1 and "in place" in L.ga_last_error().decode()
    for b in bufs:
        b.assert_unchanged("operand")


def test_engine_three_device_steps():
    """DiLoCoOuterAdam on one process, K = 3 in place: each step checked from the
    state read back before it, t and the bias corrections advancing."""
    from gym_amd.comm import Collective
    from gym_amd.engine import DiLoCoOuterAdam
    K, n = 3, N_VEC
    hp = hp_of("adamw", (0.9, 0.999))
    eng = DiLoCoOuterAdam(Collective(), K, n, DEV, torch.float32, **hp)
    master = make_state(21, n, 1)[0]
    eng.init_master(torch.from_numpy(master[:n]).to(DEV))
    reps = Buf(np.zeros((K, n), f32))
    for t in (1, 2, 3):
        pre = [bits(x).view(f32).copy() for x in (eng.master, eng.exp_avg, eng.exp_avg_sq)]
        rows = make_rows(30 + t, K, n, np.concatenate([pre[0], np.zeros(LD - n, f32)]))
        reps.rows[:, :n] = torch.from_numpy(rows).to(DEV)
        eng(reps.rows)
        assert eng.t == t and eng.launch_elems == [n] and eng.placement["placed"] is False
        got = [bits(x).view(f32) for x in (eng.master, eng.exp_avg, eng.exp_avg_sq)]
        want = C.oracle_step(rows, K, *pre, t, hp)
        print(f"engine step {t}: bit-identical shares {C.bit_shares(got, want)}")
        C.assert_step(got, want, f"engine step {t}")
        for k in range(K):
            assert np.array_equal(bits(reps.rows[k, :n]), bits(eng.master))
        reps.assert_outside_unchanged(f"engine step {t}")
    assert pre[2].any()  # step 3 started from non-zero moments
    eng.init_master(torch.from_numpy(master[:n]).to(DEV))
    assert eng.t == 0 and not bits(eng._state[n:]).any()


@pytest.mark.parametrize("bad", ["null-moment", "ld<n", "divisor-0", "bf16-state"])
def test_argument_errors_leave_every_operand_unchanged(bad):
    from gym_amd import _lib, ops
    L = _lib.lib()
    n, K = N_VEC, 2
    master, m, v = make_state(9, n, 4)
    src = Buf(make_rows(9, K, n, master))
    st = [Buf(x[None, :]) for x in (master, m, v)]
    sc = scalars(hp_of("none", (0.9, 0.999)), 4)
    if bad == "bf16-state":
        half = Buf(m[None, :], torch.bfloat16)
        with pytest.raises(TypeError, match="float32"):
            ops.diloco_outer_adam(src.rows[:, :n], st[0].rows[0], half.rows[0], st[2].rows[0], src.rows[:, :n], n, K,
                                  **sc)
        with pytest.raises(TypeError, match="float32"):
            ops.diloco_outer_adam_masked(src.rows[:, :n], packed_mask(n, 1)[1], st[0].rows[0], st[1].rows[0],
                                         half.rows[0], n, float(K), K, **sc)
        half.assert_unchanged("bf16 state")
    else:
        args = dict(ld=LD, div=float(K), m=_c(st[1].rows))
        args.update({"null-moment": dict(m=None), "ld<n": dict(ld=n - 4), "divisor-0": dict(div=0.0)}[bad])
        rc = L.ga_diloco_outer_adam(0, _c(src.rows), K, args["ld"], n, args["div"], _c(st[0].rows), args["m"],
                                    _c(st[2].rows), *[float(x) for x in sc.values()], _c(src.rows), K, args["ld"],
                                    None)
        assert rc == 1 and L.ga_last_error().decode().startswith("ga_diloco_outer_adam:")
    for b in st + [src]:
        b.assert_unchanged(f"{bad}: operand")
