"""Every path of ga_diloco_outer_islands on the MI355X, bit for bit against the numpy
oracle (tests/island_checks.py).  A workgroup covers 1024 vectors or 1024 scalars of one
island: n = 8200 (ld = n + 8) is the vector path with three workgroups per island, the
last two vectors long; n = 2135 (ld = n + 9) the element path with three workgroups;
n = 4096 with every base pointer one element off alignment the element path forced by
misalignment; n = 4 and n = 1 the smallest launches.  Across them the tables: S = 5 with
islands [[0, 3], [1, 2, 4]] in place (x aliases src; non-contiguous, ragged), one island
of 9 (past the member unroll of 8), an island of one, the process pattern (3 gathered
rows, slots [-1, 0, -1], a separate x, K_state = 1) and S = 6 with K_state = 4, two of
three islands passed with mixed -1 slots; fp32 and bf16, first and later steps, Nesterov,
dampening, no momentum with a null buffer, weight decay on and off.  Every buffer is
longer than the kernel is told and the rest holds a sentinel that must be bit-unchanged,
as must the rows no slot names.  Every local member's master, momentum and x row also
equal those of a ga_diloco_outer launch over a scratch copy of its island's rows.
Inputs are finite."""
import numpy as np
import pytest
import torch

import island_checks as I
import quant_checks as Q

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
SENT = -7.25

NEST = dict(lr=0.7, momentum=0.9, nesterov=True, dampening=0.0)
DAMP = dict(lr=0.5, momentum=0.8, nesterov=False, dampening=0.1)
NOMOM = dict(lr=0.7, momentum=0.0, nesterov=False, dampening=0.0)

# name -> (S, K_state, islands, slots, x aliases src)
TABLES = {
    "inplace5": (5, 5, [[0, 3], [1, 2, 4]], [[0, 3], [1, 2, 4]], True),
    "nine": (9, 9, [list(range(9))], [list(range(9))], True),
    "one": (3, 3, [[1]], [[1]], True),
    "process": (3, 1, [[0, 1, 2]], [[-1, 0, -1]], False),
    "mixed": (6, 4, [[0, 2, 5], [1, 4]], [[0, -1, -1], [-1, 3]], False),  # the island [3] is not passed
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gym_amd import _lib
    _lib.lib()


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu()


def _bits(t):
    """Bit patterns of a host tensor (fp32 -> int32, bf16 -> int16)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _set(rows, ld, values, dtype, off):
    """A [rows, ld] sentinel-filled device set, its base `off` elements past an aligned one,
    holding `values` [rows, n] in its first n columns."""
    t = torch.full((rows * ld + off,), SENT, device=DEV, dtype=dtype)[off:].view(rows, ld)
    t[:, :values.shape[1]] = torch.from_numpy(values).to(DEV).to(dtype)
    return t


CASES = [
    # n, ld - n, table, bf16, first, hp, wd, off
    (8200, 8, "inplace5", False, 0, NEST, 1e-3, 0),
    (8200, 8, "inplace5", True, 1, DAMP, 0.0, 0),
    (8200, 8, "nine", False, 0, DAMP, 0.0, 0),
    (8200, 8, "nine", True, 0, NEST, 1e-3, 0),
    (8200, 8, "one", False, 1, NEST, 0.0, 0),
    (8200, 8, "process", False, 0, NEST, 0.0, 0),
    (8200, 8, "process", True, 0, NOMOM, 1e-3, 0),
    (8200, 8, "mixed", False, 0, NEST, 1e-3, 0),
    (8200, 8, "mixed", True, 1, NEST, 0.0, 0),
    (8200, 8, "inplace5", False, 0, NOMOM, 0.0, 0),
    (2135, 9, "inplace5", False, 0, NEST, 1e-3, 0),
    (2135, 9, "nine", True, 1, NEST, 0.0, 0),
    (2135, 9, "one", True, 0, DAMP, 1e-3, 0),
    (2135, 9, "process", False, 1, DAMP, 0.0, 0),
    (2135, 9, "mixed", False, 0, NOMOM, 0.0, 0),
    (4096, 8, "inplace5", False, 0, NEST, 1e-3, 1),   # every base pointer one element off alignment
    (4096, 8, "process", True, 0, NEST, 0.0, 1),
    (4096, 8, "mixed", False, 1, DAMP, 1e-3, 1),
    (4, 4, "inplace5", False, 0, NEST, 1e-3, 0),
    (4, 4, "process", True, 1, NEST, 0.0, 0),
    (1, 7, "mixed", True, 0, DAMP, 0.0, 0),
    (1, 7, "nine", False, 0, NOMOM, 0.0, 0),
]


def _id(c):
    n, pad, table, bf16, first, hp, wd, off = c
    kind = "nomom" if hp is NOMOM else ("damp" if hp is DAMP else "nest")
    return (f"n{n}-{table}-{'bf16' if bf16 else 'f32'}-{'first' if first else 'later'}-{kind}-wd{wd}"
            f"{'-off1' if off else ''}")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_islands_match_the_oracle_and_the_per_member_outer_step(case):
    from gym_amd import ops
    n, pad, table, bf16, first, hp, wd, off = case
    S, Ks, islands, slots, alias = TABLES[table]
    hp = dict(hp, weight_decay=wd)
    ld = n + pad
    dtype = torch.bfloat16 if bf16 else torch.float32
    rng = np.random.default_rng(2000 + n + 10 * S + Ks)
    base = (rng.standard_normal(n) * 0.02).astype(f32)
    master = (base + rng.standard_normal((Ks, n)) * 1e-3).astype(f32)  # every node its own master
    mom = (rng.standard_normal((Ks, n)) * 1e-3).astype(f32)
    src = (base + rng.standard_normal((S, n)) * 1e-3).astype(f32)
    live = (base + rng.standard_normal((Ks, n)) * 2e-3).astype(f32)
    if bf16:
        src, live = Q.bf16_round(src), Q.bf16_round(live)
    if alias:
        assert S == Ks and slots == islands
        live = src
    has_mom = hp["momentum"] != 0
    named = sorted(v for sl in slots for v in sl if v >= 0)
    unnamed = [k for k in range(Ks) if k not in named]

    want_m, want_b, want_x = I.step(src, islands, slots, master, mom if has_mom else None, hp, bool(first), bf16)
    assert sorted(want_x) == named
    assert np.isfinite(want_m).all() and all(not np.array_equal(want_m[k], master[k]) for k in named)

    # the composite of the existing kernels, per local member: a scratch copy of its island's rows, ga_diloco_outer
    ref = {}
    for members, sl in zip(islands, slots):
        for slot in sl:
            if slot < 0:
                continue
            scratch = _set(len(members), ld, src[members], dtype, 0)
            r_m = torch.from_numpy(master[slot]).to(DEV)
            r_b = torch.from_numpy(mom[slot]).to(DEV) if has_mom else None
            r_x = torch.full((n,), SENT, device=DEV, dtype=dtype)
            ops.diloco_outer(scratch, r_m, r_b, r_x, n, float(len(members)), hp["lr"], hp["momentum"],
                             hp["dampening"], hp["weight_decay"], hp["nesterov"], bool(first))
            ref[slot] = (_host(r_m), _host(r_b) if has_mom else None, _host(r_x))

    d_src = _set(S, ld, src, dtype, off)
    d_x = d_src if alias else _set(Ks, ld, live, dtype, off)
    d_m = _set(Ks, ld, master, torch.float32, off)
    d_b = _set(Ks, ld, mom, torch.float32, off) if has_mom else None
    if off:
        assert d_src.data_ptr() % 8 and d_m.data_ptr() % 16 and d_x.data_ptr() % 8

    ops.diloco_outer_islands(d_src, islands, slots, d_m, d_b, d_x, n, hp["lr"], hp["momentum"], hp["dampening"],
                             hp["weight_decay"], hp["nesterov"], bool(first))

    got_m = _host(d_m)
    assert np.array_equal(_bits(got_m[:, :n]), want_m.view(np.int32)), "master"
    assert (got_m[:, n:] == SENT).all()
    assert np.array_equal(_bits(got_m[unnamed, :n]), master[unnamed].view(np.int32)), "rows no slot names"
    if has_mom:
        got_b = _host(d_b)
        assert np.array_equal(_bits(got_b[:, :n]), want_b.view(np.int32)), "momentum"
        assert (got_b[:, n:] == SENT).all()
        assert np.array_equal(_bits(got_b[unnamed, :n]), mom[unnamed].view(np.int32))
    got_src = _host(d_src)
    assert (got_src[:, n:].float() == SENT).all()
    if not alias:
        assert np.array_equal(_bits(got_src[:, :n]), Q.to_dtype_bits(src, bf16)), "the sources are only read"
    got_x = _host(d_x)
    assert (got_x[:, n:].float() == SENT).all()
    for k in named:
        assert np.array_equal(_bits(got_x[k, :n]), Q.to_dtype_bits(want_x[k], bf16)), ("row", k)
        assert not np.array_equal(_bits(got_x[k, :n]), Q.to_dtype_bits(live[k], bf16)), "the row changed"
        r_m, r_b, r_x = ref[k]
        assert torch.equal(r_m, got_m[k, :n]), ("master against ga_diloco_outer", k)
        if has_mom:
            assert torch.equal(r_b, got_b[k, :n]), ("momentum against ga_diloco_outer", k)
        assert np.array_equal(_bits(r_x), _bits(got_x[k, :n])), ("row against ga_diloco_outer", k)
    assert np.array_equal(_bits(got_x[unnamed, :n]), Q.to_dtype_bits(live[unnamed], bf16)), "rows no slot names"


def test_ops_wrapper_checks_its_arguments():
    from gym_amd import ops
    n = 64
    x = torch.zeros(2, n, device=DEV)
    m, b = torch.zeros(2, n, device=DEV), torch.zeros(2, n, device=DEV)
    isl = [[0, 1]]
    args = (0.7, 0.9, 0.0, 0.0, True, False)
    with pytest.raises(ValueError, match="shorter than n"):
        ops.diloco_outer_islands(x, isl, isl, m[:, :32], b, x, n, *args)
    with pytest.raises(ValueError, match="shorter than n"):
        ops.diloco_outer_islands(x, isl, isl, m, b, x[:, :32], n, *args)
    with pytest.raises(TypeError, match="dtype mismatch"):
        ops.diloco_outer_islands(x, isl, isl, m, b, x.bfloat16(), n, *args)
    with pytest.raises(TypeError, match="float32"):
        ops.diloco_outer_islands(x, isl, isl, m.bfloat16(), b, x, n, *args)
    with pytest.raises(ValueError, match="state rows"):
        ops.diloco_outer_islands(x, isl, isl, m[:1], b[:1], x, n, *args)
    with pytest.raises(ValueError, match="momentum buffer"):
        ops.diloco_outer_islands(x, isl, isl, m, None, x, n, *args)
    with pytest.raises(ValueError, match="used twice"):
        ops.diloco_outer_islands(x, [[0], [1]], [[0], [0]], m, b, x, n, *args)
    torch.cuda.synchronize()
    assert not x.any() and not m.any()  # nothing ran
