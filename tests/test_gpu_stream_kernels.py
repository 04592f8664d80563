"""Every path of the streaming kernels behind the headline number
(ga_diloco_outer, ga_replica_mean, ga_adam_step, ga_grad_clip_coef and the three
placement probes) against the oracle, at the smallest shapes that span their
work split: one workgroup owns 1024 vectors or 1024 scalars, so the vector path
runs n = 2*4096 + 4*37 = 8340 and the scalar path n = 2*1024 + 37 = 2085 (two
full workgroups and a partial one each).

Every buffer is allocated longer than the kernel is told (row stride ld > n,
master / momentum with 64 elements behind n) and the rest holds a sentinel that
must be bit-unchanged afterwards.  Bars: same-order fp32 bit-exact; the fp32
outer step at the bars of test_gpu_kernels.test_diloco_outer_matches_oracle;
bf16 results equal to the fp32 oracle rounded once to bf16 (torch's
`.bfloat16()`, round to nearest even) in >= 0.999 of the elements and within one
bf16 ulp in the rest (a 1-ulp fp32 difference flips a bf16 rounding only at a
tie; truncation would miss about half of the elements).
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import diloco as odiloco
from oracle import reduce as oreduce
# buffers inside sentinel-filled allocations and the Adam / clip bars, shared with test_gpu_sgd_kernel.py
from sgd_kernel_checks import (DEV, LD_ADAM, N_ADAM, SENT, Placed, adam_data, adam_hp, bits, check_adam_replica,
                               check_clip, host)

pytestmark = pytest.mark.gpu

f32 = np.float32
N_VEC = 2 * 4096 + 4 * 37  # 8340: 2085 vectors = two full workgroups + 37 vectors
N_SCALAR = 2 * 1024 + 37   # 2085: odd, so the launcher takes the scalar kernels


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gym_amd import _lib
    _lib.lib()


def rounded_bf16_bits(x):
    """fp32 oracle result rounded once to bf16 by torch, as int16 bit patterns."""
    return torch.from_numpy(np.ascontiguousarray(x, f32)).bfloat16().view(torch.int16).numpy()


def bf16_ulps(a, b):
    """|a - b| in bf16 units in the last place, from int16 bit patterns."""
    def key(x):
        x = x.astype(np.int32) & 0xffff
        mag = x & 0x7fff
        return np.where(x & 0x8000, -mag, mag)
    return np.abs(key(a) - key(b))


def assert_bf16_rounded_once(got_bits, want_f32, what):
    want = rounded_bf16_bits(want_f32)
    share = float((got_bits == want).mean())
    worst = int(bf16_ulps(got_bits, want).max())
    print(f"{what}: share equal to the oracle rounded once to bf16 = {share:.6f}, worst = {worst} bf16 ulp")
    assert share >= 0.999 and worst <= 1, (what, share, worst)


# ---------------------------------------------------------------- DiLoCo ------
HP = dict(lr=0.7, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=True)


def outer_data(n, K, seed, noise=1e-3):
    rng = np.random.default_rng(seed)
    master = (rng.standard_normal(n) * 0.02).astype(f32)
    reps = (master + rng.standard_normal((K, n)) * noise).astype(f32)
    mom = (rng.standard_normal(n) * 1e-3).astype(f32)
    return master, reps, mom


def run_outer(src, master, mom, dst, n, divisor, first, **hp):
    from gym_amd import ops
    h = {**HP, **hp}
    ops.diloco_outer(src, master, mom, dst, n, divisor, h["lr"], h["momentum"], h["dampening"], h["weight_decay"],
                     h["nesterov"], first)


def want_outer(master, mom, reps, first, divisor=None, **hp):
    h = {**HP, **hp}
    m, b, _ = odiloco.outer_step(master, None if first else mom, list(reps), h["lr"], h["momentum"], h["nesterov"],
                                 h["dampening"], h["weight_decay"], divisor)
    return m, b


def check_outer_fp32(gm, gb, want_m, want_b, master0):
    """The bars of test_gpu_kernels.test_diloco_outer_matches_oracle."""
    np.testing.assert_allclose(gm, want_m, rtol=1e-6, atol=1e-9)
    if want_b is not None:
        np.testing.assert_allclose(gb, want_b, rtol=0, atol=1e-6 * np.abs(master0).max())
    assert (gm == want_m).mean() >= 0.999


@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("K", [1, 3])
def test_diloco_scalar_path_by_length(K, first, nesterov):
    """diloco_outer_kernel<float, float, false> chosen by n % 4 != 0."""
    n = N_SCALAR
    master, reps, mom = outer_data(n, K, 100 + K)
    S, D = Placed(reps, ld=n + 12), Placed(np.zeros((K, n)), ld=n + 12)
    M, B = Placed(master), Placed(np.zeros(n) if first else mom)
    run_outer(S.view, M.view, B.view, D.view, n, K, first, nesterov=nesterov)
    want_m, want_b = want_outer(master, mom, reps, first, nesterov=nesterov)
    check_outer_fp32(M.data(), B.data(), want_m, want_b, master)
    assert all(np.array_equal(row, M.data_bits()) for row in D.data_bits())
    assert S.untouched() and D.outside_untouched() and M.outside_untouched() and B.outside_untouched()


@pytest.mark.parametrize("alias", [False, True], ids=["dst-apart", "dst-is-src"])
@pytest.mark.parametrize("n", [N_VEC, N_SCALAR], ids=["vec", "scalar"])
def test_diloco_writes_nothing_past_n(n, alias):
    """Row stride n + 12 and master / momentum of n + 64 elements: the sentinels behind
    every row and behind n are bit-unchanged (the vector path stores through buffer
    descriptors with a 2 GiB range, so the hardware clips nothing)."""
    K = 3
    master, reps, mom = outer_data(n, K, 7)
    S, M, B = Placed(reps, ld=n + 12), Placed(master), Placed(mom)
    D = S if alias else Placed(np.zeros((K, n)), ld=n + 12)
    run_outer(S.view, M.view, B.view, D.view, n, K, False)
    want_m, want_b = want_outer(master, mom, reps, False)
    check_outer_fp32(M.data(), B.data(), want_m, want_b, master)
    assert all(np.array_equal(row, M.data_bits()) for row in D.data_bits())
    assert S.outside_untouched() and D.outside_untouched() and M.outside_untouched() and B.outside_untouched()
    assert alias or S.untouched()


@functools.lru_cache(maxsize=None)
def _outer_aligned():
    """The aligned (vector path) run every misaligned run must reproduce bit for bit."""
    n, K = N_VEC, 3
    master, reps, mom = outer_data(n, K, 11)
    S, D, M, B = Placed(reps, ld=n + 12), Placed(np.zeros((K, n)), ld=n + 12), Placed(master), Placed(mom)
    run_outer(S.view, M.view, B.view, D.view, n, K, False)
    return (master, reps, mom), (M.data_bits(), B.data_bits(), D.data_bits())


def test_diloco_aligned_run_matches_oracle():
    (master, reps, mom), (gm, gb, gd) = _outer_aligned()
    want_m, want_b = want_outer(master, mom, reps, False)
    check_outer_fp32(gm.view(f32), gb.view(f32), want_m, want_b, master)
    assert all(np.array_equal(row, gm) for row in gd)


@pytest.mark.parametrize("which", ["src", "dst", "master", "mom", "ld_src"])
def test_diloco_scalar_path_by_alignment_bit_identical(which):
    """One operand 4 bytes off 16-byte alignment (or an odd src row stride) sends the
    same data through the scalar kernel: the per-element arithmetic is the same
    explicit fmaf chain, so the result is bit-identical to the aligned run."""
    (master, reps, mom), (am, ab, ad) = _outer_aligned()
    n, K = N_VEC, 3
    off = {which: 1}
    S = Placed(reps, ld=n + 13 if which == "ld_src" else n + 12, off=off.get("src", 0))
    D = Placed(np.zeros((K, n)), ld=n + 12, off=off.get("dst", 0))
    M, B = Placed(master, off=off.get("master", 0)), Placed(mom, off=off.get("mom", 0))
    if which != "ld_src":
        assert {"src": S, "dst": D, "master": M, "mom": B}[which].view.data_ptr() % 16 == 4
    run_outer(S.view, M.view, B.view, D.view, n, K, False)
    assert np.array_equal(M.data_bits(), am) and np.array_equal(B.data_bits(), ab)
    assert np.array_equal(D.data_bits(), ad)
    assert S.untouched() and D.outside_untouched() and M.outside_untouched() and B.outside_untouched()


@pytest.mark.parametrize("with_buffer", [False, True], ids=["mom-none", "mom-buffer-ignored"])
@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("n", [N_VEC, N_SCALAR], ids=["vec", "scalar"])
def test_diloco_without_momentum(n, wd, with_buffer):
    """momentum = 0 (DiLoCoOuter allocates no momentum then): plain SGD on the
    pseudo-gradient, against the oracle and torch.optim.SGD (fp32, single-tensor; the
    bars of test_diloco_outer_dampening_weight_decay_vs_torch_sgd); a momentum buffer
    passed anyway is not touched."""
    K = 3
    master, reps, _ = outer_data(n, K, 21)
    hp = dict(momentum=0.0, nesterov=False, weight_decay=wd)
    S, D, M = Placed(reps, ld=n + 12), Placed(np.zeros((K, n)), ld=n + 12), Placed(master)
    B = Placed(np.full(n, 3.5)) if with_buffer else None
    run_outer(S.view, M.view, B.view if B else None, D.view, n, K, True, **hp)
    want_m, want_b = want_outer(master, None, reps, True, **hp)
    assert want_b is None
    check_outer_fp32(M.data(), None, want_m, None, master)
    ref = torch.nn.Parameter(torch.from_numpy(master.copy()))
    opt = torch.optim.SGD([ref], lr=0.7, momentum=0.0, weight_decay=wd, foreach=False)
    ref.grad = torch.from_numpy(master - oreduce.mean_reduce(list(reps)))
    opt.step()
    np.testing.assert_allclose(M.data(), ref.detach().numpy(), rtol=1e-6, atol=1e-8)
    assert all(np.array_equal(row, M.data_bits()) for row in D.data_bits())
    assert S.untouched() and D.outside_untouched() and M.outside_untouched()
    assert B is None or B.untouched()


@pytest.mark.parametrize("n", [N_VEC, N_SCALAR], ids=["vec", "scalar"])
def test_diloco_without_dst(n):
    """dst=None (K_out = 0): master and momentum are updated, src is only read."""
    K = 3
    master, reps, mom = outer_data(n, K, 31)
    S, M, B = Placed(reps, ld=n + 12), Placed(master), Placed(mom)
    run_outer(S.view, M.view, B.view, None, n, K, False)
    want_m, want_b = want_outer(master, mom, reps, False)
    check_outer_fp32(M.data(), B.data(), want_m, want_b, master)
    assert S.untouched() and M.outside_untouched() and B.outside_untouched()


@pytest.mark.parametrize("n", [N_VEC, N_SCALAR], ids=["vec", "scalar"])
def test_diloco_summed_src_into_replica_rows(n):
    """The engines' cross-process shape: a 1-D summed src, divisor = the total node
    count, the new master written to every local replica row (K = 1, K_out = 5)."""
    master, reps, mom = outer_data(n, 8, 41)
    summed = oreduce.mean_reduce(list(reps), divisor=1)
    S, D, M, B = Placed(summed), Placed(np.zeros((5, n)), ld=n + 12), Placed(master), Placed(mom)
    run_outer(S.view, M.view, B.view, D.view, n, 8.0, False)
    want_m, want_b = want_outer(master, mom, [summed], False, divisor=8.0)
    check_outer_fp32(M.data(), B.data(), want_m, want_b, master)
    assert all(np.array_equal(row, M.data_bits()) for row in D.data_bits())
    assert S.untouched() and D.outside_untouched() and M.outside_untouched() and B.outside_untouched()


@pytest.mark.parametrize("n", [N_VEC, N_SCALAR], ids=["vec", "scalar"])
def test_diloco_replica_rows_into_one_dst(n):
    """K = 3 replicas, K_out = 1: a 1-D dst."""
    master, reps, mom = outer_data(n, 3, 51)
    S, D, M, B = Placed(reps, ld=n + 12), Placed(np.zeros(n)), Placed(master), Placed(mom)
    run_outer(S.view, M.view, B.view, D.view, n, 3, False)
    want_m, want_b = want_outer(master, mom, reps, False)
    check_outer_fp32(M.data(), B.data(), want_m, want_b, master)
    assert np.array_equal(D.data_bits(), M.data_bits())
    assert S.untouched() and D.outside_untouched() and M.outside_untouched() and B.outside_untouched()


@pytest.mark.parametrize("first", [True, False])
def test_diloco_shard_form(first):
    """DiLoCoOuter._outer_shard's call: a 1-D reduce-scattered src for the master range
    [m0, m1), master / momentum slices at m0 > 0, dst a slice of a parameter row.  The
    range equals the same range of a whole-buffer call bit for bit and the three
    neighbouring quarters of master, momentum and the row are bit-unchanged."""
    q = 2112
    N, m0, m1 = 4 * q, q, 2 * q
    master, reps, mom = outer_data(N, 8, 61)
    summed = oreduce.mean_reduce(list(reps), divisor=1)
    row = np.full(N, 1.25, f32)
    Sw, Dw, Mw, Bw = Placed(summed), Placed(row), Placed(master), Placed(mom)
    run_outer(Sw.view[:N], Mw.view[:N], Bw.view[:N], Dw.view[:N], N, 8.0, first)
    S, D, M, B = Placed(summed[m0:m1]), Placed(row), Placed(master), Placed(mom)
    run_outer(S.view[:q], M.view[m0:m1], B.view[m0:m1], D.view[m0:m1], q, 8.0, first)
    want_m, want_b = want_outer(master, mom, [summed], first, divisor=8.0)
    check_outer_fp32(Mw.data(), Bw.data(), want_m, want_b, master)
    keep = np.ones(M.buf.numel(), bool)
    keep[m0:m1] = False
    for part, whole in ((M, Mw), (B, Bw), (D, Dw)):
        got = bits(part.buf)
        assert np.array_equal(got[m0:m1], bits(whole.buf)[m0:m1])
        assert np.array_equal(got[keep], part.before[keep])
    assert np.array_equal(bits(D.buf)[m0:m1], bits(M.buf)[m0:m1]) and S.untouched()


@pytest.mark.parametrize("master_dtype", [torch.float32, torch.bfloat16], ids=["master-f32", "master-bf16"])
@pytest.mark.parametrize("n", [N_VEC, N_SCALAR], ids=["vec", "scalar"])
def test_diloco_bf16_rounds_once_to_nearest_even(n, master_dtype):
    """<bf16, float, *> and <bf16, bf16, *>: inputs rounded to bf16 first, the fp32
    oracle on those values, the result rounded once to bf16 (an fp32 master stays fp32
    at the fp32 bars).  Measured on the MI355X: share equal to the rounded oracle
    1.000000 (worst 0 bf16 ulp) for master, momentum and every dst row, in all four
    cases."""
    K, bf = 3, torch.bfloat16
    master, reps, mom = outer_data(n, K, 71, noise=1e-2)
    S, D = Placed(reps, ld=n + 12, dtype=bf), Placed(np.zeros((K, n)), ld=n + 12, dtype=bf)
    M, B = Placed(master, dtype=master_dtype), Placed(mom, dtype=master_dtype)
    master_in, mom_in, reps_in = M.data(), B.data(), S.data()  # the values the kernel reads
    run_outer(S.view, M.view, B.view, D.view, n, K, False)
    want_m, want_b = want_outer(master_in, mom_in, reps_in, False)
    tag = f"diloco bf16 n={n} master={'f32' if master_dtype == torch.float32 else 'bf16'}"
    if master_dtype == torch.float32:
        check_outer_fp32(M.data(), B.data(), want_m, want_b, master_in)
    else:
        assert_bf16_rounded_once(M.data_bits(), want_m, tag + " master")
        assert_bf16_rounded_once(B.data_bits(), want_b, tag + " momentum")
    for k, row in enumerate(D.data_bits()):
        assert_bf16_rounded_once(row, want_m, tag + f" dst[{k}]")
        assert np.array_equal(row, D.data_bits()[0])
    assert S.untouched() and D.outside_untouched() and M.outside_untouched() and B.outside_untouched()


# ---------------------------------------------------------------- mean --------
@pytest.mark.parametrize("n,ld,K,rows,K_out", [
    (N_VEC, N_VEC + 12, 2, None, 1), (N_VEC, N_VEC + 12, 5, None, 1), (1001, 1013, 3, None, 1),
    (N_VEC, N_VEC + 12, 5, [4, 1, 3], 1), (1001, 1013, 5, [4, 1, 3], 1), (N_VEC, N_VEC + 12, 5, None, 3),
    (1001, 1013, 2, None, 3)],
    ids=["vec-K2", "vec-K5", "scalar-odd-ld", "vec-rows", "scalar-rows", "vec-Kout3", "scalar-Kout3"])
def test_replica_mean_bf16_bit_exact(n, ld, K, rows, K_out):
    """bf16 mean: ascending fp32 sum and a true division (nothing to reorder), rounded
    once to bf16: bit-exact against the oracle, `rows` summed in the given order."""
    from gym_amd import ops
    bf = torch.bfloat16
    x = np.random.default_rng(n + K).standard_normal((K, n)).astype(f32)
    S, D = Placed(x, ld=ld, dtype=bf), Placed(np.zeros((K_out, n)), ld=ld + 4, dtype=bf)
    r = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=DEV)
    ops.replica_mean(S.view, D.view, n=n, rows=r)
    want = rounded_bf16_bits(oreduce.mean_reduce(list(S.data()), rows=rows))
    assert all(np.array_equal(row, want) for row in D.data_bits())
    assert S.untouched() and D.outside_untouched()


@functools.lru_cache(maxsize=None)
def _mean_aligned():
    from gym_amd import ops
    n, K = N_VEC, 3
    x = np.random.default_rng(81).standard_normal((K, n)).astype(f32)
    S, D = Placed(x, ld=n + 12), Placed(np.zeros((2, n)), ld=n + 12)
    ops.replica_mean(S.view, D.view, n=n)
    return x, D.data_bits()


@pytest.mark.parametrize("which", ["aligned", "src", "dst", "ld_src", "ld_dst"])
def test_replica_mean_fp32_misaligned_bit_identical(which):
    from gym_amd import ops
    x, aligned = _mean_aligned()
    n = N_VEC
    assert all(np.array_equal(row.view(f32), oreduce.mean_reduce(list(x))) for row in aligned)
    S = Placed(x, ld=n + 13 if which == "ld_src" else n + 12, off=int(which == "src"))
    D = Placed(np.zeros((2, n)), ld=n + 13 if which == "ld_dst" else n + 12, off=int(which == "dst"))
    ops.replica_mean(S.view, D.view, n=n)
    assert np.array_equal(D.data_bits(), aligned)
    assert S.untouched() and D.outside_untouched()


# ---------------------------------------------------------------- probes ------
SPECIAL_BITS = (0x80000000, 0x00000001, 0x807fffff, 0x7fc01234, 0x7f800001, 0xffc00000, 0x7f800000, 0xff800000)


def bit_soup(numel, seed):
    """An fp32 device buffer of distinct ordinary values with -0.0, denormals, quiet and
    signalling NaN payloads and infinities planted (built and compared as int32)."""
    u = np.random.default_rng(seed).standard_normal(numel).astype(f32).view(np.uint32).copy()
    for j, s in enumerate(SPECIAL_BITS):
        u[(j * 523 + 3) % numel::4099] = s
    return torch.from_numpy(u.view(np.int32)).to(DEV)


def soup_rows(K, n, ld, seed):
    raw = bit_soup(K * ld + 64, seed)
    return raw, raw[:K * ld].view(torch.float32).view(K, ld)[:, :n]


@pytest.mark.parametrize("probe", ["diloco", "mean"])
@pytest.mark.parametrize("K", [1, 3, 16])
def test_outer_and_mean_probes_leave_every_byte_unchanged(K, probe):
    """The engines run the placement probes on live training state: every allocated
    byte (replicas, their padding, master / momentum and what lies behind n) equals its
    copy taken before, compared as int32."""
    from gym_amd import ops
    n, ld = N_VEC, N_VEC + 12
    R, reps = soup_rows(K, n, ld, 1000 + K)
    M, B = bit_soup(n + 64, 2000 + K), bit_soup(n + 64, 3000 + K)
    before = [x.clone() for x in (R, M, B)]
    assert not torch.equal(M, B) and all(not torch.equal(reps[k].view(torch.int32), M[:n]) for k in range(K))
    assert all(not torch.equal(reps[k], reps[0]) for k in range(1, K))
    if probe == "diloco":
        ops.probe_diloco_placement(reps, n, M.view(torch.float32), B.view(torch.float32))
    else:
        ops.probe_mean_placement(reps, n)
    torch.cuda.synchronize()
    for got, want in zip((R, M, B), before):
        assert torch.equal(got, want)


@pytest.mark.parametrize("K", [1, 3])
def test_adam_probe_leaves_every_byte_unchanged(K):
    from gym_amd import ops
    n, ld = N_VEC, N_VEC + 12
    raws, views = zip(*(soup_rows(K, n, ld, 4000 + 10 * K + i) for i in range(4)))
    before = [x.clone() for x in raws]
    assert all(not torch.equal(raws[i], raws[j]) for i in range(4) for j in range(i))
    ops.probe_adam_placement(*views)
    torch.cuda.synchronize()
    for got, want in zip(raws, before):  # parameters, gradients, both moments
        assert torch.equal(got, want)


# ---------------------------------------------------------------- clip --------
N_CLIP = 4 * 262144 + 4 * 1000 + 3  # 1 052 579: a second grid-stride trip and a 3-element scalar tail


@functools.lru_cache(maxsize=None)
def _clip_rows():
    x = np.random.default_rng(91).standard_normal((3, N_CLIP)).astype(f32)
    x *= (f32(0.01) * np.array([0.01, 1.0, 100.0], f32))[:, None]  # norms ~ 0.1, 10, 1000
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("ld", [N_CLIP + 5, N_CLIP + 6], ids=["ld-n+5", "ld-odd"])
def test_clip_coef_three_replicas_two_trips(ld, dtype):
    """sumsq_kernel over K = 3 rows (blockIdx.y row and partials offsets), 263 144
    vectors against a grid stride of 262 144 (second trip) plus a scalar tail.  Row
    stride n + 5 is a multiple of 4, so every row takes the vector loop; the odd stride
    n + 6 leaves rows 1 and 2 misaligned, which take the scalar-only loop (nv = 0).
    Replica 0 does not clip (coefficient exactly 1), replicas 1 and 2 do."""
    from gym_amd import ops
    G = Placed(_clip_rows(), ld=ld, dtype=dtype)
    part, out = ops.sumsq_partials(DEV, 3), torch.full((6,), SENT, device=DEV)
    ops.grad_clip_coef(G.view, N_CLIP, 1.0, part, out)
    got = check_clip(out, G.data().astype(np.float64), 1.0)
    assert got[0] == 1.0 and got[2] < 1.0 and got[4] < 1.0
    assert G.untouched()


@pytest.mark.parametrize("n", [3, 257])
def test_clip_coef_tiny_and_zero_gradients(n):
    from gym_amd import ops
    x = np.random.default_rng(n).standard_normal((2, n)).astype(f32)
    G = Placed(x, ld=n + 5)
    part, out = ops.sumsq_partials(DEV, 2), torch.full((4,), SENT, device=DEV)
    ops.grad_clip_coef(G.view, n, 0.5, part, out)
    check_clip(out, x.astype(np.float64), 0.5)
    Z = Placed(np.zeros((2, n)), ld=n + 5)
    ops.grad_clip_coef(Z.view, n, 0.5, part, out)
    assert np.array_equal(host(out), np.array([1.0, 0.0, 1.0, 0.0], f32))  # the sentinels behind n are not summed
    assert G.untouched() and Z.untouched()


# ---------------------------------------------------------------- Adam --------
# N_ADAM = 8343, LD_ADAM = 8352: 2085 float4 = two workgroups + a partial one, and a 3-element tail
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.3, 0.9)], ids=["beta1-0.9", "beta1-0.3"])
@pytest.mark.parametrize("step", [1, 4])
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam-l2"])
def test_adam_step_three_replicas_direct(decoupled, step, betas):
    """ga_adam_step called directly on [3, 8352] sets with n = 8343, non-zero moments and
    per-replica clip coefficients; betas (0.3, 0.9) takes lerp's weight >= 0.5 form.
    Measured on the MI355X: p, m and v bit-identical to the oracle in a share of
    1.000000 of the elements, every replica of all eight variants."""
    from gym_amd import ops
    K, n, ld = 3, N_ADAM, LD_ADAM
    start = adam_data(200 + step)
    sets = [Placed(x, ld=ld) for x in start]
    part, out = ops.sumsq_partials(DEV, K), torch.zeros(2 * K, device=DEV)
    ops.grad_clip_coef(sets[1].view, n, 1.0, part, out)
    lr, eps, wd = 1e-3, 1e-8, (1e-2 if decoupled else 0.05)
    ops.adam_step(*(s.view for s in sets), clip_coef=out, **adam_hp(lr, betas, eps, wd, decoupled, step))
    coefs = host(out)[0::2]
    assert coefs[0] == 1.0 and coefs[1] < 1.0 and coefs[2] < 1.0
    got = [s.data() for s in sets]
    kw = dict(lr=lr, betas=betas, eps=eps, weight_decay=wd, decoupled=decoupled)
    for k in range(K):
        check_adam_replica([x[k] for x in got], [x[k] for x in start], float(coefs[k]), step, kw,
                           f"adam {'adamw' if decoupled else 'l2'} step {step} betas {betas} replica {k}")
    assert all(s.outside_untouched() for s in sets)  # columns [n, ld) and the pad of all four sets


def test_adam_step_refuses_bad_geometry_before_launching():
    """A misaligned set, or a row stride that is no multiple of 4 at K > 1, raises from
    the host check; nothing is launched (all four sets bit-unchanged)."""
    from gym_amd import ops
    from gym_amd._lib import HipLibraryError
    hp = adam_hp(1e-3, (0.9, 0.999), 1e-8, 1e-2, True, 1)
    for K, ld, off in ((3, N_ADAM + 10, 0), (3, LD_ADAM, 1), (1, None, 1)):
        start = adam_data(300, K=K)
        for bad in range(4 if off else 1):
            sets = [Placed(x, ld=ld, off=off if i == bad else 0) for i, x in enumerate(start)]
            with pytest.raises(HipLibraryError):
                ops.adam_step(*(s.view for s in sets), **hp)
            assert all(s.untouched() for s in sets)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_adam_nonfinite_gradient_parity_with_torch(bad):
    """clip_grad_norm_ with a non-finite total norm (clamp(nan, max=1) is nan): one NaN
    gradient element makes the replica's coefficient, norm, whole gradient, parameters
    and moments NaN, exactly where clip_grad_norm_ + AdamW on the CPU put NaN; one +inf
    gives coefficient 0: zero gradients and one NaN.  The neighbouring replicas meet the
    ordinary bars."""
    from gym_amd import ops
    K, n, ld = 3, N_ADAM, LD_ADAM
    start = adam_data(400, zero_state=True)
    start[1][1, 4321] = bad
    sets = [Placed(x, ld=ld) for x in start]
    part, out = ops.sumsq_partials(DEV, K), torch.zeros(2 * K, device=DEV)
    ops.grad_clip_coef(sets[1].view, n, 1.0, part, out)
    lr, betas, eps, wd = 1e-3, (0.9, 0.999), 1e-8, 1e-2
    ops.adam_step(*(s.view for s in sets), clip_coef=out, **adam_hp(lr, betas, eps, wd, True, 1))
    o = host(out)
    got = [s.data() for s in sets]
    if math.isnan(bad):
        assert np.isnan(o[2]) and np.isnan(o[3])
    else:
        assert o[2] == 0.0 and np.isposinf(o[3])
    # the reference on the CPU
    ref_p = torch.nn.Parameter(torch.from_numpy(start[0][1].copy()))
    ref_p.grad = torch.from_numpy(start[1][1].copy())
    opt = torch.optim.AdamW([ref_p], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    torch.nn.utils.clip_grad_norm_([ref_p], 1.0)
    ref_g = ref_p.grad.numpy().copy()
    opt.step()
    ref = (ref_p.detach().numpy(), ref_g, opt.state[ref_p]["exp_avg"].numpy(), opt.state[ref_p]["exp_avg_sq"].numpy())
    for name, x, r in zip("pgmv", got, ref):
        print(f"{name}: NaN on the device {int(np.isnan(x[1]).sum())}, in torch {int(np.isnan(r).sum())} of {n}")
        assert np.array_equal(np.isnan(x[1]), np.isnan(r))
        assert int(np.isnan(r).sum()) == (n if math.isnan(bad) else 1)
        np.testing.assert_allclose(x[1], r, rtol=1e-5, atol=1e-7, equal_nan=True)
    kw = dict(lr=lr, betas=betas, eps=eps, weight_decay=wd, decoupled=True)
    for k in (0, 2):
        check_adam_replica([x[k] for x in got], [x[k] for x in start], float(o[2 * k]), 1, kw, f"replica {k}")
    assert all(s.outside_untouched() for s in sets)
