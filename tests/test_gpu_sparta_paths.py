"""Every path of the SPARTA kernels (gym_amd/csrc/sparta.hip) that the oracle
comparisons of test_gpu_kernels.py leave out, bit for bit against oracle.sparta's masks
and tests/sparta_checks.py's expected values (pinned on the CPU by
tests/test_sparta_checks.py):

  A. the K x source x dtype matrix of the wave kernels: K in {4, 8, 16, 32, 64}, each of
     the four mask sources, fp32 and bf16 -- the wave average, the wave select + V4
     scatter, the V4 tile-gather with the list; several list windows at p = 0.6;
  B. designed selection counts per 4096-element wave tile (0, 1, 255, 256, 257, 4096,
     513, 63 and a ragged tail; a sparse 16384 tile beside one over kSelCap), as a bits
     mask and as a byte mask with values other than 0/1, lists cut by cap;
  C. (in test_gpu_kernels.py) the bf16 tests compare bits;
  D. divisors that are no power of two on the wave kernels, subnormal averages, and
     the second rounding of select -> scatter in bf16 (invisible at divisor = K);
  E. the high words of the Philox iteration and seed and of torch's generator offset;
  F. the device {seed, offset} pair (seedoff) of both draw kernels and the in-kernel draw;
  G. the tile-gather kernel's K > kGatherSlots one-lane loop, K == kSlots, the rows
     layout beyond the rows wave kernel, the V4 size limit, a misaligned base;
  H. runs of tensors smaller than a 64-element group under the in-kernel draw;
  I. the scan kernel's second pass (more than 16384 count tiles).

Every replica buffer carries sentinel padding (spare rows and columns for element-major
sets, a spare tail for rows) that must come back untouched, and so do the packed lists
past their counts.  Which kernel a case reaches is reasoned from launch_select's
conditions ("SPARTA paths and their tests").
"""
import functools

import numpy as np
import pytest
import torch

from oracle import sparta as osparta
import sparta_checks as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
SENT, IDX_SENT, VAL_SENT = 7.0, -7, -3.0       # replica padding, idx and vals past the count
PAD_ROWS, PAD_TAIL = 3, 61                     # spare rows of an element-major buffer, spare tail of rows
N0 = 2 * 16384 + 4096 + 77                     # three count tiles, the last a partial wave tile with a ragged group
SEED, ITER = 0x1234_5678_9ABC, 17


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gym_amd import _lib
    _lib.lib()


def _bits(x):
    """Integer view of a tensor's bits (bitwise comparisons: -0 != +0, NaN == NaN)."""
    return x.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[x.element_size()])


def _same(got, want):
    """got (device tensor) holds exactly the float32 array `want` in its own dtype."""
    w = torch.from_numpy(np.ascontiguousarray(want, dtype=np.float32)).to(got.dtype)
    assert np.array_equal(sc.bits_of(w.float().numpy()), sc.bits_of(want)), "expected values are not in the dtype"
    return torch.equal(_bits(got.contiguous().cpu()), _bits(w))


@functools.lru_cache(None)
def _x(K, n, seed=0, scale=1.0):
    """[K, n] float32 replicas (row k = replica k); shared, never modified."""
    a = np.random.default_rng(1000 * K + seed).standard_normal((K, n), dtype=np.float32) * np.float32(scale)
    a.setflags(write=False)
    return a


def _full(want, n, layout, ld=None, col0=0):
    """The whole buffer of a replica set holding want [K, n]: element-major [n + PAD_ROWS,
    ld] with the set in columns col0 .. col0 + K, or rows [K, n + PAD_TAIL]; SENT elsewhere."""
    K = want.shape[0]
    if layout == "elem":
        full = np.full((n + PAD_ROWS, K if ld is None else ld), SENT, np.float32)
        full[:n, col0:col0 + K] = want[:, :n].T
    else:
        full = np.full((K, n + PAD_TAIL), SENT, np.float32)
        full[:, :n] = want[:, :n]
    return full


def _dev_set(x, n, dtype, layout, ld=None, col0=0):
    """(buffer, replica set view) on the device for the replicas x [K, n]."""
    buf = torch.from_numpy(_full(x, n, layout, ld, col0)).to(DEV, dtype)
    return buf, (buf[:, col0:col0 + x.shape[0]] if layout == "elem" else buf)


def _list_bufs(n, size, dtype):
    from gym_amd import ops
    return dict(idx=torch.full((size,), IDX_SENT, dtype=torch.int32, device=DEV),
                vals=torch.full((size,), VAL_SENT, dtype=dtype, device=DEV),
                count=torch.full((2,), -1, dtype=torch.int64, device=DEV), work=ops.sparta_workspace(n, DEV))


def _check_list(L, sel, want_vals, cap, what):
    """count = {selected, overflow}; the first min(cap, selected) entries of idx / vals;
    everything after them keeps its sentinel."""
    k = min(cap, len(sel))
    c = L["count"].cpu().numpy()
    assert c[0] == len(sel) and c[1] == int(len(sel) > cap), (what, c, len(sel), cap)
    idx = L["idx"].cpu().numpy()
    assert np.array_equal(idx[:k], sel[:k]), what
    assert (idx[k:] == IDX_SENT).all(), what
    assert _same(L["vals"][:k], want_vals[:k]), what
    assert _same(L["vals"][k:], np.full(L["vals"].numel() - k, VAL_SENT, np.float32)), what


def _check_paths(x, n, m, kw, dtype, divisor, paths, layout="elem", ld=None, col0=0, cap=None, what=""):
    """Runs the named paths on fresh copies of the replicas x [K, n] under the mask m
    (kw: the mask arguments of the ops wrappers) and compares every bit:
      "avg"      sparta_average_local without the list -> expect_fused;
      "avg_list" sparta_average_local with idx / vals / count -> expect_fused (every
                 selected element, whatever cap), vals = RN_dtype(fp32 sum);
      "select"   sparta_select, then sparta_scatter of the listed entries -> expect_two_step.
    Returns the resulting buffers by path."""
    from gym_amd import ops
    sel = np.flatnonzero(m)
    cap = len(sel) + 8 if cap is None else cap
    size = cap + 8                                  # entries past cap: never written
    fused = sc.expect_fused(x, m, divisor, dtype)
    want_vals, _ = sc.expect_two_step(x, m, divisor, dtype)
    out = {}
    for path in paths:
        tag = (what, path, layout, x.shape[0], str(dtype), divisor, cap)
        buf, view = _dev_set(sc.round_to(x, dtype), n, dtype, layout, ld, col0)
        if path == "avg":
            ops.sparta_average_local(view, n, divisor, layout=layout, **kw)
            assert _same(buf, _full(fused, n, layout, ld, col0)), tag
        elif path == "avg_list":
            L = _list_bufs(n, size, dtype)
            ops.sparta_average_local(view, n, divisor, layout=layout, cap=cap, **L, **kw)
            assert _same(buf, _full(fused, n, layout, ld, col0)), tag
            _check_list(L, sel, want_vals, cap, tag)
        else:
            assert path == "select", path
            L = _list_bufs(n, size, dtype)
            ops.sparta_select(view, n, cap, L["idx"], L["vals"], L["count"], L["work"], layout=layout, **kw)
            assert _same(buf, _full(sc.round_to(x, dtype), n, layout, ld, col0)), tag   # select only reads
            _check_list(L, sel, want_vals, cap, tag)
            ops.sparta_scatter(L["vals"], L["idx"], L["count"], cap, divisor, view, layout=layout)
            listed = np.zeros(m.size, bool)
            listed[sel[:cap]] = True
            _, two = sc.expect_two_step(x, listed, divisor, dtype)
            assert _same(buf, _full(two, n, layout, ld, col0)), tag
        out[path] = buf
    return out


# ---------------------------------------------------------------- mask sources ---
BYTE_VALUES = (1, 2, 0x80, 0xFF)


def _bytes_mask(m, values=(1,)):
    """uint8 arena of the bool mask m, set bytes cycling through `values`; 64 set bytes
    past n that no kernel may read as selections."""
    b = m.astype(np.uint8) * np.resize(np.array(values, np.uint8), m.size)
    assert np.array_equal(b != 0, m)
    return torch.from_numpy(np.concatenate([b, np.full(64, 0xFF, np.uint8)])).to(DEV)


def _bits_mask(m):
    """int64 packed words of m, the last word's bits past n set (the kernels mask them)."""
    w = osparta.pack_mask(m).view(np.uint64).copy()
    if m.size % 64:
        w[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(m.size % 64)
    return torch.from_numpy(w.view(np.int64)).to(DEV)


T_SEED, T_OFF = 1234, 24


@functools.lru_cache(None)
def _source(kind, n, p, seed=SEED, it=ITER):
    """(bool mask, mask keyword arguments of the ops wrappers) of a mask source: the
    Philox stream, a byte mask, a bits mask, the in-kernel reference draw of one n-element
    tensor at generator offset 24."""
    from gym_amd import ops
    if kind == "philox":
        return osparta.philox_mask(n, seed, it, p), dict(seed=seed, iteration=it, p=p)
    if kind == "torch":
        table, _ = ops.sparta_bernoulli_table([0], [n], DEV)
        return (osparta.torch_gpu_bernoulli(n, p, T_SEED, T_OFF),
                dict(mask=ops.TorchDraw(table, p, T_SEED, T_OFF, 12)))
    m = np.random.default_rng(n + int(p * 1000)).random(n) < p
    return m, dict(mask=_bytes_mask(m) if kind == "bytes" else _bits_mask(m))


# ------------------------------------------- A. K x source x dtype of the wave kernels ---
A_CASES = ([(K, s, 0.05) for K in (4, 8, 16, 32, 64) for s in ("philox", "bytes", "bits", "torch")] +
           [(16, "philox", 0.6), (4, "bytes", 0.6), (64, "bits", 0.6), (8, "torch", 0.6)])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("K,source,p", A_CASES)
def test_wave_kernels_K_source_dtype_matrix(K, source, p, dtype):
    """Element-major ld = K: sparta_average_wave_kernel<T, K/4, SRC> (WaveBatchDpp, or
    WaveBatchDpp2 under the reference draw at K >= 8), sparta_select_wave_kernel + the V4
    scatter, and sparta_select_kernel<T, true> with the list.  p = 0.6 lists ~2450
    selections per wave tile: ten kWList windows."""
    m, kw = _source(source, N0, p)
    assert m.any() and not m.all()
    _check_paths(_x(K, N0), N0, m, kw, DTYPES[dtype], float(K), ("avg", "select", "avg_list"))


# ---------------------------------------------------------------- B. designed counts ---
B_COUNTS = [0, 1, 255, 256, 257, 4096, 513, 63]
NB = 8 * 4096 + 77
B_FORMS = {
    "wave-avg-K4": dict(K=4, paths=("avg",)),                     # one batch of 128 per window
    "wave-avg-K64": dict(K=64, paths=("avg",)),                   # eight batches of 32 per window
    "wave-select-K4": dict(K=4, paths=("select",)),
    "wave-select-K64": dict(K=64, paths=("select",)),
    "rows-wave-K3": dict(K=3, paths=("avg",), layout="rows"),
    "rows-list-K3": dict(K=3, paths=("avg_list",), layout="rows"),          # tile-gather, per_pass = 256
    "elem-list-K12-ld14": dict(K=12, paths=("avg_list",), ld=14),           # tile-gather, per_pass = 157
}


@functools.lru_cache(None)
def _designed(kind):
    m = sc.mask_with_tile_counts(B_COUNTS, 4096, 77)
    assert m.size == NB and int(m[:16384].sum()) == 512 and int(m[16384:32768].sum()) == 4929
    return m, dict(mask=_bits_mask(m) if kind == "bits" else _bytes_mask(m, BYTE_VALUES))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["bits", "bytes"])
@pytest.mark.parametrize("form", list(B_FORMS))
def test_designed_counts_per_wave_tile(form, kind, dtype):
    """Exactly 0 / 1 / 255 / 256 / 257 / 4096 / 513 / 63 selections in the 4096-element
    wave tiles (kWList = 256 windows full, one short, one over; a whole tile; the per-wave
    pos0 prefix of the wave select), 512 and 4929 (> kSelCap) in the two 16384 tiles, every
    element of the ragged tail.  Byte masks hold 1, 2, 0x80 and 0xFF.  The list forms run
    again at cap = 700, inside the 257-count tile: the overflow flag is set, the first 700
    entries are right and nothing is written after them."""
    f = dict(B_FORMS[form])
    K, paths = f.pop("K"), f.pop("paths")
    m, kw = _designed(kind)
    _check_paths(_x(K, NB, seed=1), NB, m, kw, DTYPES[dtype], float(K), paths, what=form, **f)
    if paths != ("avg",):
        _check_paths(_x(K, NB, seed=1), NB, m, kw, DTYPES[dtype], float(K), paths, cap=700, what=form, **f)


# ---------------------------------------------------------------- D. divisors ---------
D_FORMS = {"elem-K8-philox": (8, "elem", "philox"), "elem-K8-torch": (8, "elem", "torch"),
           "elem-K32-philox": (32, "elem", "philox"), "elem-K32-torch": (32, "elem", "torch"),
           "rows-K8-philox": (8, "rows", "philox")}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("form", list(D_FORMS))
def test_divisors_that_are_not_the_replica_count(form, dtype):
    """The averages are the correctly rounded fp32 quotients for any positive divisor:
    3, 12 and 2.5 take the true division of WaveBatchDpp (Philox) and div_nodes
    (WaveBatchDpp2, reference draw), 32 and 0.5 the reciprocal multiply of div_nodes."""
    K, layout, source = D_FORMS[form]
    m, kw = _source(source, N0, 0.05)
    for divisor in (3.0, 12.0, 2.5, 32.0, 0.5):
        _check_paths(_x(K, N0, seed=2), N0, m, kw, DTYPES[dtype], divisor, ("avg",), layout=layout, what=form)


@pytest.mark.parametrize("K,source", [(8, "philox"), (32, "torch")])
def test_exchange_path_rounds_twice_in_bf16(K, source):
    """With the replica count as divisor the scatter's quotient of a bf16 value is exact
    and its rounding invisible.  Divisors 3 and 12 make the second rounding real: select
    stores RN_bf16(fp32 sum), the V4 scatter packs RN_bf16(vals / divisor), which differs
    from the fused one-rounding result at some elements; the V4 tile-gather with the list
    rounds once."""
    m, kw = _source(source, N0, 0.05)
    x = _x(K, N0, seed=2)
    for divisor in (3.0, 12.0):
        fused = sc.expect_fused(x, m, divisor, torch.bfloat16)
        two = sc.expect_two_step(x, m, divisor, torch.bfloat16)[1]
        assert 0 < (fused[0] != two[0]).sum() < m.sum()       # the two contracts are told apart
        _check_paths(x, N0, m, kw, torch.bfloat16, divisor, ("select", "avg_list"))


@pytest.mark.parametrize("form", list(D_FORMS))
def test_subnormal_averages_are_kept(form):
    """fp32 inputs scaled by 2^-140: sums and averages are subnormal.  The pin: torch's
    own true division on this GPU (tensor by tensor; a Python scalar divisor would become
    a multiply by the rounded 1/d in torch) keeps subnormals and equals numpy's fp32
    division bit for bit, so the kernels' multiply by 1/32 and their division by 12 must too."""
    K, layout, source = D_FORMS[form]
    m, kw = _source(source, N0, 0.05)
    x = _x(K, N0, seed=3, scale=2.0 ** -140)
    sums = sc.expect_two_step(x, m, 1.0, torch.float32)[0]
    assert (np.abs(sums) < np.float32(2.0 ** -126)).all() and (sums != 0).mean() > 0.9
    for divisor in (32.0, 12.0):
        want = (sums / np.float32(divisor)).astype(np.float32)
        assert (want != 0).mean() > 0.5
        pin = torch.from_numpy(sums).to(DEV) / torch.full((sums.size,), divisor, device=DEV)
        print(f"{form} / {divisor}: torch differs from numpy at {(pin.cpu().numpy() != want).sum()} of {want.size}")
        assert _same(pin, want)                                           # the pin
        _check_paths(x, N0, m, kw, torch.float32, divisor, ("avg",), layout=layout, what=form)


# ---------------------------------------------------------------- E. high counter words -
HI_SEED, HI_ITER = 0xABCDEF0123456789, (7 << 32) + 5
HI_TSEED, HI_TOFF = 0xFEDCBA9876543210, 2 ** 34 + 24


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("K,layout,paths", [(32, "elem", ("avg",)), (3, "rows", ("avg",)), (8, "elem", ("select",))])
def test_philox_high_words_of_iteration_and_seed(K, layout, paths, dtype):
    """iteration >= 2^32 (Pred::it_hi) and a seed with high bits, on the wave average, the
    rows wave average and the exchange select (count, scan and wave select kernels)."""
    p = 0.05
    m = osparta.philox_mask(N0, HI_SEED, HI_ITER, p)
    assert (m != osparta.philox_mask(N0, HI_SEED, 5, p)).sum() > 100            # the high word matters
    assert (m != osparta.philox_mask(N0, HI_SEED & 0xFFFFFFFF, HI_ITER, p)).sum() > 100
    kw = dict(seed=HI_SEED, iteration=HI_ITER, p=p)
    _check_paths(_x(K, N0, seed=4), N0, m, kw, DTYPES[dtype], float(K), paths, layout=layout)


@functools.lru_cache(None)
def _hi_torch_mask(n, p):
    m = osparta.torch_gpu_bernoulli(n, p, HI_TSEED, HI_TOFF)
    assert (m != osparta.torch_gpu_bernoulli(n, p, HI_TSEED, 24)).sum() > 100    # offset's high word
    assert (m != osparta.torch_gpu_bernoulli(n, p, HI_TSEED & 0xFFFFFFFF, HI_TOFF)).sum() > 100
    return m


def _draw_both_formats(table, nb, base, n, p, seed, off0, seedoff=None):
    """ga_sparta_torch_bernoulli of one n-element tensor at arena offset `base` (a
    multiple of 64), bytes and bits: (bool mask from the bytes, from the bits); checks
    the bytes are 0/1 and everything outside the tensor is untouched."""
    from gym_amd import ops
    size = base + n + 64
    by = torch.full((size,), 9, dtype=torch.uint8, device=DEV)
    ops.sparta_torch_bernoulli(table, nb, p, seed, off0, 12, by, seedoff=seedoff)
    g = by.cpu().numpy()
    assert (g[:base] == 9).all() and (g[base + n:] == 9).all() and set(np.unique(g[base:base + n])) <= {0, 1}
    words = ops.sparta_mask_words(size)
    bi = torch.full((words,), -1, dtype=torch.int64, device=DEV)
    ops.sparta_torch_bernoulli(table, nb, p, seed, off0, 12, bi, seedoff=seedoff)
    w = bi.cpu().numpy()
    w0, w1 = base // 64, base // 64 + -(-n // 64)
    assert (w[:w0] == -1).all() and (w[w1:] == -1).all()
    if n % 64:
        assert int(w[w1 - 1].view(np.uint64)) >> (n % 64) == 0               # tail bits past numel are zero
    return g[base:base + n] != 0, osparta.unpack_mask(w[w0:w1], n)


def test_reference_draw_kernels_high_offset_and_seed():
    """ga_sparta_torch_bernoulli, bytes (the {ctr lo, ctr hi} counter of its own Philox
    call) and bits (torch_ctr's ctr >> 32 term), at generator offset 2^34 + 24 and a
    seed with high bits."""
    from gym_amd import ops
    p = 0.05
    want = _hi_torch_mask(N0, p)
    table, nb = ops.sparta_bernoulli_table([64], [N0], DEV)
    got_bytes, got_bits = _draw_both_formats(table, nb, 64, N0, p, HI_TSEED, HI_TOFF)
    assert np.array_equal(got_bytes, want)
    assert np.array_equal(got_bits, want)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("K", [4, 16])
def test_in_kernel_draw_high_offset_and_seed(K, dtype):
    """The same generator state through TorchDraw: the wave average at K = 4
    (WaveBatchDpp under the reference draw) and K = 16 (WaveBatchDpp2)."""
    from gym_amd import ops
    p = 0.05
    table, _ = ops.sparta_bernoulli_table([0], [N0], DEV)
    kw = dict(mask=ops.TorchDraw(table, p, HI_TSEED, HI_TOFF, 12))
    _check_paths(_x(K, N0, seed=5), N0, _hi_torch_mask(N0, p), kw, DTYPES[dtype], float(K), ("avg",))


def test_torch_stream_at_a_high_offset_pins_the_oracle():
    """torch.bernoulli(torch.full(...)) itself at generator offset 2^34 + 24 against
    oracle.sparta.torch_gpu_bernoulli, where this torch build's generator accepts such an
    offset (if set_offset refuses it, torch cannot reach that state and the oracle
    comparisons above stand alone)."""
    gen = torch.cuda.default_generators[0]
    saved = torch.cuda.get_rng_state()
    try:
        torch.manual_seed(777)
        try:
            gen.set_offset(HI_TOFF)
        except (RuntimeError, OverflowError, ValueError) as e:
            print(f"generator.set_offset(2**34 + 24) refused: {e}")
            return
        assert gen.get_offset() == HI_TOFF
        numel, p = 4096 * 3 + 2, 0.05
        want = torch.bernoulli(torch.full((numel,), p, device=DEV)).bool().cpu().numpy()
        assert gen.get_offset() == HI_TOFF + 12
        assert np.array_equal(osparta.torch_gpu_bernoulli(numel, p, gen.initial_seed(), HI_TOFF), want)
        print("generator.set_offset(2**34 + 24) accepted: oracle pinned against torch.bernoulli")
    finally:
        torch.cuda.set_rng_state(saved)


# ---------------------------------------------------------------- F. seedoff ----------
SO_SEED, SO_OFF = 0xF123456789ABCDEF, 2 ** 34 + 48      # a seed above 2^63: int64 two's complement on the device
HOST_SEED, HOST_OFF = 1, 48                             # the host arguments, which must be ignored


def _seedoff():
    from gym_amd.strategy.sparta import _i64
    assert _i64(SO_SEED) < 0
    return torch.tensor([_i64(SO_SEED), _i64(SO_OFF)], dtype=torch.int64, device=DEV)


@functools.lru_cache(None)
def _seedoff_mask(n, p):
    m = osparta.torch_gpu_bernoulli(n, p, SO_SEED, SO_OFF)
    assert (m != osparta.torch_gpu_bernoulli(n, p, HOST_SEED, HOST_OFF)).sum() > 100
    return m


def test_reference_draw_kernels_read_the_device_seed_and_offset():
    """ga_sparta_torch_bernoulli with seedoff, both formats: the masks of the device
    {seed, offset}, not of the seed / offset0 arguments."""
    from gym_amd import ops
    p = 0.05
    table, nb = ops.sparta_bernoulli_table([64], [N0], DEV)
    got_bytes, got_bits = _draw_both_formats(table, nb, 64, N0, p, HOST_SEED, HOST_OFF, seedoff=_seedoff())
    assert np.array_equal(got_bytes, _seedoff_mask(N0, p))
    assert np.array_equal(got_bits, _seedoff_mask(N0, p))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("K,layout", [(32, "elem"), (3, "rows")])
def test_in_kernel_draw_reads_the_device_seed_and_offset(K, layout, dtype):
    """TorchDraw(seedoff=...) through the wave average and the rows wave average
    (torch_bits64's tseedoff branch)."""
    from gym_amd import ops
    p = 0.05
    table, _ = ops.sparta_bernoulli_table([0], [N0], DEV)
    kw = dict(mask=ops.TorchDraw(table, p, HOST_SEED, HOST_OFF, 12, seedoff=_seedoff()))
    _check_paths(_x(K, N0, seed=6), N0, _seedoff_mask(N0, p), kw, DTYPES[dtype], float(K), ("avg",), layout=layout)


# ---------------------------------------------------------------- G. tile-gather branches
NG, PG = 3000, 0.02
G_FORMS = {
    "elem-K2049-one-lane-loop": dict(K=2049, layout="elem"),        # non-V4 (K odd), K > kGatherSlots
    "rows-K2048-one-entry-per-pass": dict(K=2048, layout="rows"),   # K == kSlots: Kp = Ki, per_pass = 1
    "rows-K130-beyond-rows-wave": dict(K=130, layout="rows"),       # > 4 kRowsKB: per_pass = 2048 / 131 = 15
    "elem-K3072-v4-limit": dict(K=3072, layout="elem"),             # V4, K == kGatherSlotsV4
    "elem-K3076-v4-refused": dict(K=3076, layout="elem"),           # K % 4 == 0 but > kGatherSlotsV4: one-lane loop
}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("form", list(G_FORMS))
def test_tile_gather_branches(form, dtype):
    """sparta_select_kernel's branches by K, without the list (tile_offsets == NULL) and
    with it; n = 3000 in one tile, the Philox source."""
    f = G_FORMS[form]
    m = osparta.philox_mask(NG, SEED, ITER, PG)
    assert 20 < m.sum() < 200
    kw = dict(seed=SEED, iteration=ITER, p=PG)
    _check_paths(_x(f["K"], NG, seed=7), NG, m, kw, DTYPES[dtype], float(f["K"]), ("avg", "avg_list"),
                 layout=f["layout"], what=form)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_element_major_base_not_vector_aligned(dtype):
    """K = 32 as columns 1..32 of an [n, 40] buffer: K and the stride are multiples of 4
    but the base is not 4-element aligned, so the vector forms are refused
    (sparta_select_kernel<T, false>, scalar scatter).  Bit-identical to the aligned run
    (columns 0..31), with and without the list and through select + scatter; columns 0
    and 33..39 untouched."""
    K = 32
    m = osparta.philox_mask(NG, SEED, ITER, PG)
    kw = dict(seed=SEED, iteration=ITER, p=PG)
    paths = ("avg", "avg_list", "select")
    mis = _check_paths(_x(K, NG, seed=8), NG, m, kw, DTYPES[dtype], float(K), paths, ld=40, col0=1)
    ali = _check_paths(_x(K, NG, seed=8), NG, m, kw, DTYPES[dtype], float(K), paths, ld=40, col0=0)
    for path in paths:
        assert torch.equal(_bits(mis[path][:, 1:33].contiguous()), _bits(ali[path][:, 0:32].contiguous())), path
        assert (mis[path][:, 0] == SENT).all() and (mis[path][:, 33:] == SENT).all(), path


# ---------------------------------------------------------------- H. tiny tensors ------
@functools.lru_cache(None)
def _tiny_arena(p):
    """150 tensors of 1, 3, 63, 64, 65, 5, ... elements at 64-aligned offsets from 128 on,
    every seventh not drawn (padding groups inside waves), then one of 5000 elements:
    (n, bool mask, draw table, offset of the last tensor).  Drawn tensor i uses generator offset T_OFF + 12 i."""
    from gym_amd import ops
    numels = [(1, 3, 63, 64, 65, 5)[j % 6] for j in range(150)] + [5000]
    offs, o = [], 128
    for nel in numels:
        offs.append(o)
        o += -(-nel // 64) * 64
    n = o + 17                                   # a few undrawn elements after the last tensor
    drawn = [j for j in range(len(numels)) if j % 7 != 5]
    assert drawn[0] == 0 and offs[0] == 128 and drawn[-1] == 150
    m = np.zeros(n, bool)
    for i, j in enumerate(drawn):
        m[offs[j]:offs[j] + numels[j]] = osparta.torch_gpu_bernoulli(numels[j], p, T_SEED, T_OFF + 12 * i)
    table, _ = ops.sparta_bernoulli_table([offs[j] for j in drawn], [numels[j] for j in drawn], DEV)
    return n, m, table, offs[-1]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("K,layout,paths", [(32, "elem", ("avg",)), (3, "rows", ("avg",)), (8, "elem", ("select",))])
def test_in_kernel_draw_over_runs_of_tiny_tensors(K, layout, paths, dtype):
    """torch_bits64's tensor lookup where every lane of a wave sits in another tensor (the
    scalar search for the first lane, then a walk of up to 63 table rows), the arena's
    first 128 elements and every seventh tensor undrawn."""
    from gym_amd import ops
    p = 0.3
    n, m, table, last = _tiny_arena(p)
    assert not m[:128].any() and m[128:last].sum() > 500 and m[last:].sum() > 1000 and not m[last + 5000:].any()
    kw = dict(mask=ops.TorchDraw(table, p, T_SEED, T_OFF, 12))
    _check_paths(_x(K, n, seed=9), n, m, kw, DTYPES[dtype], float(K), paths, layout=layout)


# ---------------------------------------------------------------- I. multi-pass scan ---
def test_scan_second_pass_carries_the_running_total():
    """n = 16384^2 + 3 * 16384 + 77: 16388 count tiles, so sparta_scan_kernel stages a
    second pass of kScanChunk tiles and must carry the first pass's total into it.  One
    bf16 replica (rows, K = 1) of zeros with small integers (exact in bf16) at ~5000
    seeded positions and at both ends of the first tile, of the first pass and of the
    arena; select (idx, vals, count), then scatter with divisor 2."""
    from gym_amd import ops
    T = 16384
    n = T * T + 3 * T + 77
    rng = np.random.default_rng(12)
    pos = np.unique(np.concatenate([rng.integers(0, n, 5000), rng.integers(T * T, n, 40),
                                    [0, T - 1, T, T * T - 1, T * T, T * T + T, n - 1]])).astype(np.int64)
    assert (pos >= T * T).sum() >= 40 and (pos < T * T).sum() >= 4000
    words = np.zeros(-(-n // 64), np.uint64)
    np.bitwise_or.at(words, pos >> 6, np.uint64(1) << (pos & 63).astype(np.uint64))
    words[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)             # bits past n: masked by the kernel
    bits = torch.from_numpy(words.view(np.int64)).to(DEV)
    v = (1 + np.arange(pos.size) % 255).astype(np.float32)
    pos_t = torch.from_numpy(pos).to(DEV)
    src = torch.zeros(1, n + PAD_TAIL, dtype=torch.bfloat16, device=DEV)
    src[0, n:] = SENT
    src[0, pos_t] = torch.from_numpy(v).to(DEV, torch.bfloat16)
    cap = pos.size + 8
    L = _list_bufs(n, cap + 8, torch.bfloat16)
    ops.sparta_select(src, n, cap, L["idx"], L["vals"], L["count"], L["work"], mask=bits, layout="rows")
    _check_list(L, pos, v, cap, "select")
    ops.sparta_scatter(L["vals"], L["idx"], L["count"], cap, 2.0, src, layout="rows")
    assert _same(src[0, pos_t], v / np.float32(2))
    assert int(torch.count_nonzero(src[0, :n])) == pos.size                      # nothing else was written
    assert (src[0, n:] == SENT).all()
