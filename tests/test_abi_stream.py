"""The C ABI of the streaming outer step without a GPU: the argument checks of
ga_diloco_outer_merge, which run on the host before any launch, and the ops wrapper's
own.  The kernel: test_gpu_outer_stream_kernels.py."""
import ctypes

import pytest

_P = ctypes.c_void_p(64)
_Q = ctypes.c_void_p(64 + (1 << 20))
N = 300


def _lib():
    from gym_amd import _lib
    return _lib.lib()


def test_symbol_and_version():
    from gym_amd import _lib, ops
    assert "ga_diloco_outer_merge" in _lib.header_symbols() and "ga_diloco_outer_merge" in _lib.SIGNATURES
    assert callable(ops.diloco_outer_merge)
    assert _lib.lib().ga_abi_version() == 103


def _merge(L, dtype=0, src=_P, K=2, ld_src=N, n=N, div=2.0, master=_P, mom=_P, first=0, lr=0.7, momentum=0.9,
           dampening=0.0, wd=0.0, nesterov=1, alpha=0.5, x=_Q, K_out=2, ld_x=N):
    return L.ga_diloco_outer_merge(dtype, src, K, ld_src, n, div, master, mom, first, lr, momentum, dampening, wd,
                                   nesterov, alpha, x, K_out, ld_x, None)


@pytest.mark.parametrize("bad", [
    dict(src=None), dict(master=None), dict(x=None), dict(mom=None), dict(n=-1), dict(K=0), dict(K=-2),
    dict(K_out=-1), dict(div=0.0), dict(ld_src=N - 1), dict(ld_x=N - 1), dict(dampening=0.1),
    dict(momentum=0.0, mom=None), dict(momentum=-0.5), dict(dtype=7), dict(dtype=2),
    dict(alpha=1.0), dict(alpha=-0.25), dict(alpha=1.5), dict(alpha=float("nan")), dict(alpha=float("inf")),
    dict(x=_P, K_out=1), dict(x=_P, K_out=3), dict(x=_P, ld_x=N + 4),  # aliasing src, but not the same set
])
def test_invalid_arguments_fail_cleanly(bad):
    L = _lib()
    assert _merge(L, **bad) == 1  # GA_EINVAL, checked on the host before any launch
    assert "ga_diloco_outer_merge" in L.ga_last_error().decode()


def test_zero_length_is_a_noop():
    L = _lib()
    assert _merge(L, n=0, src=None, master=None, mom=None, x=None) == 0
    assert L.ga_last_error().decode() == ""
    assert _merge(L, n=0, K_out=0, alpha=0.0) == 0 and L.ga_last_error().decode() == ""
    assert _merge(L, n=0, alpha=1.0) == 1 and _merge(L, n=0, K=0) == 1  # ...but not a licence for a bad alpha or K


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from gym_amd import ops
    x, m = torch.zeros(2, N), torch.zeros(N)
    args = (N, 2.0, 0.7, 0.0, 0.0, 0.0, False, True)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.diloco_outer_merge(x, m, None, x, *args, 0.5)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.diloco_outer_merge(x, m, None, None, *args, 0.0)
