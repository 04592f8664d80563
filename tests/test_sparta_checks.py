"""Pins tests/sparta_checks.py (the expected values of tests/test_gpu_sparta_paths.py
and of the bf16 SPARTA tests of tests/test_gpu_kernels.py) on the CPU."""
import numpy as np
import pytest
import torch

import sparta_checks as sc

BF16, F32 = torch.bfloat16, torch.float32


def test_bf16_round_is_nearest_even_on_ties():
    # bf16 has 8 significand bits: the spacing in [1, 2) is 2^-7, a tie sits at odd multiples of 2^-8
    x = np.array([1.0 + 2.0 ** -8,            # tie between 1 and 1 + 2^-7: even is 1
                  1.0 + 3 * 2.0 ** -8,        # tie between 1 + 2^-7 and 1 + 2^-6: even is 1 + 2^-6
                  1.0 + 2.0 ** -8 + 2.0 ** -23,   # just above the tie: up
                  1.0 + 2.0 ** -8 - 2.0 ** -23,   # just below: down (truncation agrees here)
                  -(1.0 + 3 * 2.0 ** -8),
                  1.0 + 2.0 ** -7 + 2.0 ** -9],   # below the tie, where truncation also gives 1 + 2^-7
                 np.float32)
    want = np.array([1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 1.0, -(1.0 + 2.0 ** -6), 1.0 + 2.0 ** -7], np.float32)
    assert np.array_equal(sc.bits_of(sc.bf16_round(x)), sc.bits_of(want))
    # truncation (the mutant the GPU tests must catch) differs on the round-up entries
    trunc = (sc.bits_of(x) & np.uint32(0xFFFF0000)).view(np.float32)
    assert (trunc != want).sum() == 3
    # already-bf16 values and subnormals pass through
    y = np.array([0.5, -3.0, 2.0 ** -133, 0.0, -0.0], np.float32)
    assert np.array_equal(sc.bits_of(sc.bf16_round(y)), sc.bits_of(y))
    assert np.array_equal(sc.bits_of(sc.round_to(x, F32)), sc.bits_of(x))


@pytest.mark.parametrize("counts,tile,tail", [([0, 1, 255, 256, 257, 4096, 513, 63], 4096, 77),
                                              ([2, 0, 64], 64, 0), ([1], 1, 3)])
def test_mask_with_tile_counts(counts, tile, tail):
    m = sc.mask_with_tile_counts(counts, tile, tail)
    assert m.dtype == bool and m.shape == (len(counts) * tile + tail,)
    for t, c in enumerate(counts):
        seg = m[t * tile:(t + 1) * tile]
        assert int(seg.sum()) == c, t
        if c >= 2:
            assert seg[0] and seg[-1], t
    assert m[len(counts) * tile:].all()
    assert np.array_equal(m, sc.mask_with_tile_counts(counts, tile, tail))          # seeded
    if max(counts) > 2 and tile > 64:
        assert not np.array_equal(m, sc.mask_with_tile_counts(counts, tile, tail, seed=1))


def test_designed_counts_per_count_tile():
    """The wave-tile counts of the GPU tests' case B give one sparse and one over-full
    16384-element count tile (kSelCap = 4096)."""
    m = sc.mask_with_tile_counts([0, 1, 255, 256, 257, 4096, 513, 63], 4096, 77)
    assert int(m[:16384].sum()) == 512 and int(m[16384:32768].sum()) == 4929 and m.size == 8 * 4096 + 77


def test_expect_fused_fp32_is_the_oracle_mean():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((5, 200)).astype(np.float32)
    m = rng.random(200) < 0.3
    out = sc.expect_fused(x, m, 5.0, F32)
    acc = np.zeros(200, np.float32)
    for k in range(5):
        acc = acc + x[k]
    assert np.array_equal(sc.bits_of(out[:, m]), sc.bits_of(np.broadcast_to((acc / np.float32(5))[m], (5, int(m.sum())))))
    assert np.array_equal(sc.bits_of(out[:, ~m]), sc.bits_of(x[:, ~m]))
    vals, out2 = sc.expect_two_step(x, m, 5.0, F32)
    assert np.array_equal(sc.bits_of(vals), sc.bits_of(acc[m])) and np.array_equal(sc.bits_of(out2), sc.bits_of(out))
    # an empty selection leaves the (rounded) inputs
    none = np.zeros(200, bool)
    assert np.array_equal(sc.expect_fused(x, none, 5.0, BF16), sc.bf16_round(x))
    v0, o0 = sc.expect_two_step(x, none, 5.0, BF16)
    assert v0.size == 0 and np.array_equal(o0, sc.bf16_round(x))


def test_two_step_differs_from_fused_in_bf16():
    """x = {1, 17 * 2^-10}: the fp32 sum 1 + 17/1024 rounds to the bf16 1 + 16/1024, and a
    third of it is 173.33 bf16 steps of 2^-9 (-> 173) where a third of the fp32 sum is
    173.5 + (-> 174): the select -> scatter path rounds twice and lands one step lower."""
    x = np.array([[1.0], [17 * 2.0 ** -10]], np.float32)
    assert np.array_equal(sc.bf16_round(x), x)
    m = np.array([True])
    fused = sc.expect_fused(x, m, 3.0, BF16)
    vals, two = sc.expect_two_step(x, m, 3.0, BF16)
    assert vals[0] == np.float32(1.015625)
    assert fused[0, 0] == fused[1, 0] == np.float32(174 * 2.0 ** -9)
    assert two[0, 0] == two[1, 0] == np.float32(173 * 2.0 ** -9)
    # in fp32 the two paths agree
    assert np.array_equal(sc.expect_fused(x, m, 3.0, F32), sc.expect_two_step(x, m, 3.0, F32)[1])


def test_division_keeps_subnormals():
    """The expected quotient is numpy's fp32 division: subnormal sums stay subnormal
    (nothing flushed to zero), correctly rounded."""
    x = np.full((4, 3), 3 * 2.0 ** -140, np.float32)
    out = sc.expect_fused(x, np.ones(3, bool), 32.0, F32)
    # 12 * 2^-140 / 32 = 3 * 2^-143
    assert out[0, 0] == np.float32(3 * 2.0 ** -143) and out[0, 0] != 0
    out = sc.expect_fused(x, np.ones(3, bool), 12.0, F32)
    assert out[0, 0] == np.float32(2.0 ** -140)
