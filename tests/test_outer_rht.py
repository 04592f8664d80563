"""The rotated integer outer step without a GPU: the outer_compression="rht-int8" | "rht-int4"
options down to engine.DiLoCoOuterRHT, the numpy oracle's transform and sign diagonal, and
the oracle's error table against the unrotated integer formats.  The kernels: test_gpu_rht.py."""
import numpy as np
import pytest
import torch

import quant_checks as Q
import rht_checks as H

f32 = np.float32
N = 700  # 3 blocks, the last one short
ROW = {8: 784, 4: 400}


@pytest.mark.parametrize("comp,bits", [("rht-int8", 8), ("rht-int4", 4)])
def test_options_build_the_rotated_engine(comp, bits, monkeypatch):
    import gym_amd.engine as engine
    from gym_amd import ops
    from gym_amd.comm import Collective
    from gym_amd.engine import RHT_FORMATS, DiLoCoOuterQuant, DiLoCoOuterRHT
    from gym_amd.strategy import DiLoCoStrategy, IslandDiLoCoStrategy, OptimSpec, SPARTADiLoCoStrategy, diloco
    monkeypatch.setattr(engine, "ops", ops)  # the library's own ops, whatever stand-in an earlier test installed
    assert RHT_FORMATS == {"rht-int8": 8, "rht-int4": 4}

    def build(s, K, n=N):
        return diloco.build_outer_engine(s, s.outer_optim_spec, Collective(), K, n, "cpu", torch.float32)
    for make in (DiLoCoStrategy, SPARTADiLoCoStrategy):
        e = build(make(outer_compression=comp), 3)
        assert type(e) is DiLoCoOuterRHT and isinstance(e, DiLoCoOuterQuant) and e.bits == bits and e.seed == 0
        assert e.residual is None and e.payload.shape == (3, ROW[bits]) and e.payload_bytes_per_node == ROW[bits]
        s = make(outer_compression=comp, outer_error_feedback=True, outer_rotation_seed=9)
        e = build(s, 2)
        assert type(e) is DiLoCoOuterRHT and e.seed == 9 and e.residual.shape == (2, N) and e.mom.numel() == N
        assert s.__config__()["outer_rotation_seed"] == 9 and make().__config__()["outer_rotation_seed"] == 0
        for bad in (True, 1.0, "1", None, -1, 2 ** 32):
            with pytest.raises(ValueError, match="outer_rotation_seed"):
                make(outer_compression=comp, outer_rotation_seed=bad)
    with pytest.raises(ValueError, match="mxfp4.*rht-int8.*rht-int4.*topk"):
        DiLoCoStrategy(outer_compression="rht-int2")
    for bad in (dict(outer_optim_spec=OptimSpec(torch.optim.Adam, lr=0.05)), dict(outer_delay=1, H=4),
                dict(outer_mix=0.5)):
        with pytest.raises(ValueError, match="outer_compression"):
            DiLoCoStrategy(outer_compression=comp, **bad)
    with pytest.raises(ValueError):
        IslandDiLoCoStrategy(outer_compression=comp)
    s = DiLoCoStrategy(outer_compression=comp, num_fragments=2, H=4, outer_rotation_seed=3)
    frag = diloco.build_streaming_outer(s, s.outer_optim_spec, Collective(), 1, 2048, "cpu", torch.float32, [0, 1024],
                                        (2, 0, 0.0))
    assert [type(e) for e in frag.engines] == [DiLoCoOuterRHT] * 2 and all(e.seed == 3 for e in frag.engines)


def test_oracle_transform_and_sign_diagonal():
    """FWHT256 is its own inverse bit for bit on integer-valued blocks (every intermediate is
    an integer below 2^24); sigma depends on (i, seed) only: a longer row starts with the
    shorter one's signs, and another seed gives other signs."""
    v = np.random.default_rng(0).integers(-127, 128, (5, 256)).astype(f32)
    y = H.fwht256(v)
    assert np.array_equal(H.fwht256(y), v) and not np.array_equal(y, v)
    assert np.array_equal(H.fwht256(np.ones(256, f32))[0], np.r_[f32(16), np.zeros(255, f32)])
    a = H.sigma(4096, 5)
    assert np.array_equal(a[:300], H.sigma(300, 5)) and set(a) == {-1.0, 1.0} and abs(a.mean()) < 0.1
    assert not np.array_equal(a, H.sigma(4096, 6)) and not np.array_equal(a[:256], a[256:512])
    # fmix32(0) = 0, so seed 0 starts with 32 plus signs; fmix32(1) is murmur3's published value
    assert (H.sigma(32, 0) == 1).all() and int(H.fmix32(np.array([1]))[0]) == 0x514E28B7


def test_error_table_against_the_unrotated_formats():
    """Oracle encode -> decode (S = 1, divisor 1, lr 1 on a zero master: the new master is
    -g) on 2^18 elements, DESIGN's two deltas.  Heavy-tailed (1% of the entries x 100):
    the rotated formats have strictly lower relative error than int8 / int4 on all entries
    and on the ordinary 99%; Gaussian: within 5% of the unrotated error."""
    n = 1 << 18
    rng = np.random.default_rng(0)
    gauss = rng.standard_normal(n).astype(f32)
    big = rng.random(n) < 0.01
    hp = dict(lr=1.0, momentum=0.0, nesterov=False, dampening=0.0, weight_decay=0.0)
    zero = np.zeros(n, f32)

    def rel(got, want, sel=slice(None)):
        return float(np.linalg.norm((got - want)[sel]) / np.linalg.norm(want[sel]))
    for bits in (8, 4):
        err = {}
        for name, d in (("gauss", gauss), ("heavy", (gauss * np.where(big, 100, 1)).astype(f32))):
            plain = -Q.decode_outer(Q.encode(zero, -d, None, bits)[0], n, bits, 1.0, zero, None, hp, True)[0]
            rot = -H.decode_outer(H.encode(zero, -d, None, bits, 0)[0], n, bits, 1.0, zero, None, hp, True, 0)[0]
            err[name], err[name + " ordinary"] = (rel(plain, d), rel(rot, d)), (rel(plain, d, ~big), rel(rot, d, ~big))
        print(f"int{bits}: (unrotated, rotated) relative error {err}")
        assert err["heavy"][1] < err["heavy"][0] and err["heavy ordinary"][1] < err["heavy ordinary"][0]
        assert abs(err["gauss"][1] - err["gauss"][0]) <= 0.05 * err["gauss"][0]
