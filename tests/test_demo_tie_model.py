"""The integer tie model behind tests/test_gpu_demo_paths.py, pinned on the CPU.

The GPU tie tests claim which branch of the wave encode's top-k they run
(chunk64_tail in gym_amd/csrc/demo_wave.hip): the fast path's tie branch for
topk in {2, 5, 7, 9}, the all-keys fallback with ties at a non-zero key for
topk = 32.  That claim rests on three facts of the constructed chunk (2^-3 at
(i, i), everything else zero), restated here in numpy: the k-th key is shared by
exactly two coefficients, one of them is needed, and the kernel's candidate count
(lane maxima -> 12-bit prefix threshold -> keys at or above it) is below / above
its capacity kCand.  If kCand or the threshold scheme changes, this fails instead
of the GPU tests silently exercising another branch.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import demo_checks
from gym_amd.demo_codec import DemoPlan, dct_table
from gym_amd.arena import ArenaLayout

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def F32():
    plan = DemoPlan(ArenaLayout([(64, 64)]))
    return plan._F64_host.numpy().copy()


def test_plan_table_is_fp32_dct_and_fold_symmetric(F32):
    """The model's table is the plan's; F[63-i][k] = (-1)^k F[i][k] holds to the bit,
    so the wave kernel's half table and the block kernel's full table agree."""
    assert np.array_equal(F32, dct_table(64).astype(np.float32))
    sgn = np.where(np.arange(64) % 2, -1.0, 1.0).astype(np.float32)
    assert np.array_equal(F32[::-1] * sgn[None, :], F32)
    assert (F32 != 0).all()


def test_kcand_matches_the_kernel():
    src = (ROOT / "gym_amd" / "csrc" / "demo_wave.hip").read_text()
    m = re.search(r"constexpr int kCand = (\d+);", src)
    assert m and int(m.group(1)) == demo_checks.KCAND
    # the 12-bit prefix threshold the model restates
    assert "for (int bit = 30; bit >= 19; --bit)" in src


@pytest.mark.parametrize("i", range(64))
def test_coefficients_are_bitwise_symmetric(F32, i):
    y = demo_checks.tie_chunk_coeffs(F32, i)
    assert np.array_equal(y.view(np.uint32), y.T.copy().view(np.uint32))
    assert np.isfinite(y).all() and (np.abs(y) >= 2.0 ** -126).all()  # no denormal: v * f * f is exact scaling


@pytest.mark.parametrize("topk", [2, 5, 7, 9])
def test_small_k_is_the_fast_path_tie_branch(F32, topk):
    for i in range(64):
        y = demo_checks.tie_chunk_coeffs(F32, i)
        idx, _, mult, need = demo_checks.topk_by_key(y, topk)
        assert (mult, need) == (2, 1), (i, mult, need)
        assert demo_checks.wave_candidate_count(y, topk) <= demo_checks.KCAND, i
        # the tie is broken towards the lower index: of the pair (b, d), (d, b) the one with b < d stays
        key = demo_checks.keys_of(y).reshape(-1)
        tied = np.flatnonzero(key == key[idx][np.argmin(key[idx])])
        assert tied.size == 2 and tied[0] in idx and tied[1] not in idx


def test_k32_is_the_fallback_with_a_non_zero_tie(F32):
    counts = []
    for i in range(64):
        y = demo_checks.tie_chunk_coeffs(F32, i)
        idx, bits, mult, need = demo_checks.topk_by_key(y, 32)
        assert (mult, need) == (2, 1), (i, mult, need)
        assert (bits & 0x7FFFFFFF).min() > 0  # the tied key is not the all-zero key
        counts.append(demo_checks.wave_candidate_count(y, 32))
    assert min(counts) > demo_checks.KCAND, counts


def test_topk_by_key_tie_rule_small_example():
    y = np.float32([0.0, -2.0, 1.0, 2.0, -1.0, 1.0, 0.0, -0.0])
    idx, bits, mult, need = demo_checks.topk_by_key(y, 3)
    assert idx.tolist() == [1, 2, 3] and (mult, need) == (3, 1)
    assert bits.tolist() == y[[1, 2, 3]].view(np.uint32).tolist()
    idx, _, mult, need = demo_checks.topk_by_key(y, 6)
    assert idx.tolist() == [0, 1, 2, 3, 4, 5] and (mult, need) == (3, 1)  # +0 and -0 tie at key 1


def test_scatter_mean_valid_is_the_oracle_when_all_valid_and_drops_the_rest():
    from oracle import demo as odemo
    rng = np.random.default_rng(0)
    S, gy, gx, k, n1, n2 = 5, 2, 3, 6, 4, 4
    idx = np.sort(rng.random((S, gy, gx, n1 * n2)).argsort(-1)[..., :k], -1)
    val = rng.standard_normal(idx.shape)
    got, cnt = demo_checks.scatter_mean_valid(idx, val, n1, n2)
    assert np.allclose(got, odemo.scatter_mean(list(idx), list(val), n1, n2), rtol=1e-15, atol=0)
    assert cnt.sum() == idx.size
    bad = idx.copy()
    bad[0, 0, 0, 0], bad[1, 1, 2, 3], bad[2, 0, 1, 2] = -1, n1 * n2, 2**31 - 1
    got2, cnt2 = demo_checks.scatter_mean_valid(bad, val, n1, n2)
    assert cnt2.sum() == idx.size - 3
    # the same as the oracle on the lists with those entries' values moved out: compare one chunk by hand
    keep = (bad[:, 0, 0] >= 0) & (bad[:, 0, 0] < n1 * n2)
    s = np.zeros(n1 * n2)
    c = np.zeros(n1 * n2)
    np.add.at(s, bad[:, 0, 0][keep], val[:, 0, 0][keep])
    np.add.at(c, bad[:, 0, 0][keep], 1)
    assert np.allclose(got2[0, 0].reshape(-1), np.where(c > 0, s / np.maximum(c, 1), 0))
