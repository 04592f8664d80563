"""The C ABI of the quantised outer step without a GPU: ga_quant_row_bytes' values
and the argument checks of ga_quant_encode / ga_diloco_outer_dequant, which run on
the host before any launch.  The kernels: test_gpu_quant_kernels.py."""
import ctypes

import pytest

import quant_checks as Q

_P = ctypes.c_void_p(64)
_ODD = ctypes.c_void_p(72)  # 8-byte aligned only
N = 300  # two blocks: 528 payload bytes at 8 bits, 272 at 4
ROW = {8: 528, 4: 272}


def _lib():
    from gym_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("n,bits,want", [(0, 8, 0), (0, 4, 0), (1, 8, 272), (1, 4, 144), (256, 8, 272), (256, 4, 144),
                                         (257, 8, 528), (257, 4, 272), (N, 8, ROW[8]), (N, 4, ROW[4])])
def test_row_bytes(n, bits, want):
    """nb * 256 * bits / 8 q bytes + nb fp32 scales, rounded up to 16."""
    assert _lib().ga_quant_row_bytes(n, bits) == want == Q.row_bytes(n, bits)
    assert want % 16 == 0


def test_row_bytes_refuses_bad_arguments_and_ops_raise():
    from gym_amd import ops
    L = _lib()
    assert L.ga_quant_row_bytes(-1, 8) == -1 and L.ga_quant_row_bytes(256, 3) == -1
    assert L.ga_quant_row_bytes(256, 16) == -1
    assert ops.quant_row_bytes(257, 4) == 272
    for bad in ((-1, 8), (16, 2)):
        with pytest.raises(ValueError, match="quant_row_bytes"):
            ops.quant_row_bytes(*bad)


def test_symbols_and_version():
    from gym_amd import _lib, ops
    syms = _lib.header_symbols()
    for name in ("ga_quant_row_bytes", "ga_quant_encode", "ga_diloco_outer_dequant"):
        assert name in syms and name in _lib.SIGNATURES
    assert callable(ops.quant_encode) and callable(ops.diloco_outer_dequant)
    assert _lib.lib().ga_abi_version() == 103


def _encode(L, dtype=0, x=_P, K=2, ld_x=N, master=_P, residual=_P, ld_r=N, n=N, bits=8, payload=_P, ld_q=None):
    ld_q = ROW.get(bits, 528) if ld_q is None else ld_q
    return L.ga_quant_encode(dtype, x, K, ld_x, master, residual, ld_r, n, bits, payload, ld_q, None)


def _dequant(L, payload=_P, S=2, ld_q=None, bits=8, n=N, div=2.0, master=_P, mom=_P, first=0, lr=0.7, momentum=0.9,
             dampening=0.0, wd=0.0, nesterov=1, dtype=0, dst=_P, K_out=2, ld_dst=N):
    ld_q = ROW.get(bits, 528) if ld_q is None else ld_q
    return L.ga_diloco_outer_dequant(payload, S, ld_q, bits, n, div, master, mom, first, lr, momentum, dampening, wd,
                                     nesterov, dtype, dst, K_out, ld_dst, None)


@pytest.mark.parametrize("bad", [
    dict(x=None), dict(master=None), dict(payload=None), dict(bits=3), dict(bits=16), dict(bits=0),
    dict(ld_q=ROW[8] - 16), dict(bits=4, ld_q=ROW[4] - 16), dict(ld_q=ROW[8] + 8), dict(payload=_ODD),
    dict(n=-1), dict(K=0), dict(K=-2), dict(ld_x=N - 1), dict(ld_r=N - 1), dict(dtype=7),
])
def test_encode_invalid_arguments_fail_cleanly(bad):
    L = _lib()
    assert _encode(L, **bad) == 1  # GA_EINVAL, checked on the host before any launch
    assert "ga_quant_encode" in L.ga_last_error().decode()


@pytest.mark.parametrize("bad", [
    dict(payload=None), dict(master=None), dict(dst=None), dict(mom=None), dict(bits=5), dict(bits=16),
    dict(ld_q=ROW[8] - 16), dict(bits=4, ld_q=ROW[4] - 16), dict(ld_q=ROW[8] + 4), dict(payload=_ODD),
    dict(n=-1), dict(S=0), dict(K_out=-1), dict(div=0.0), dict(ld_dst=N - 1), dict(dampening=0.1),
    dict(momentum=0.0, mom=None), dict(dtype=7),
])
def test_dequant_invalid_arguments_fail_cleanly(bad):
    L = _lib()
    assert _dequant(L, **bad) == 1
    assert "ga_diloco_outer_dequant" in L.ga_last_error().decode()


def test_zero_length_is_a_noop():
    L = _lib()
    assert _encode(L, n=0, x=None, master=None, residual=None, payload=None, ld_q=0) == 0
    assert L.ga_last_error().decode() == ""
    assert _dequant(L, n=0, payload=None, master=None, mom=None, dst=None, ld_q=0) == 0
    assert L.ga_last_error().decode() == ""
    assert _encode(L, n=0, bits=3) == 1 and _dequant(L, n=0, bits=3) == 1  # ...but not a licence for bad bits


def test_ops_refuse_cpu_tensors():
    import torch
    from gym_amd import ops
    x, m = torch.zeros(2, N), torch.zeros(N)
    pay = torch.zeros(2, ROW[8], dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.quant_encode(x, m, None, pay, N, 8)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.diloco_outer_dequant(pay, m, None, x, N, 8, 2.0, 0.7, 0.0, 0.0, 0.0, False, True)
