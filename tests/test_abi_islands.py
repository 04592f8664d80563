"""The C ABI of the island outer step without a GPU: the argument checks of
ga_diloco_outer_islands, which run on the host before any launch, and the ops wrapper's
own, the host-table checks among them.  The kernel: test_gpu_outer_islands_kernel.py."""
import ctypes

import pytest

_P = ctypes.c_void_p(64)
_Q = ctypes.c_void_p(64 + (1 << 20))
_T = ctypes.c_void_p(64 + (2 << 20))
N = 300
NAME = "ga_diloco_outer_islands"


def _lib():
    from gym_amd import _lib
    return _lib.lib()


def test_symbol_and_version():
    from gym_amd import _lib, ops
    assert NAME in _lib.header_symbols() and NAME in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME][1]) == 22
    assert callable(ops.diloco_outer_islands) and callable(ops.island_table)
    assert _lib.lib().ga_abi_version() == 103  # additive: the version stays
    assert ctypes.CDLL(_lib.LIB_PATH)[NAME] is not None  # exported by the built library


def _islands(L, dtype=0, src=_P, S=3, ld_src=N, n=N, starts=_T, I=2, members=_T, slots=_T, master=_Q, mom=_Q,
             K_state=2, ld_state=N, first=0, lr=0.7, momentum=0.9, dampening=0.0, wd=0.0, nesterov=1, x=_P, ld_x=N):
    return L.ga_diloco_outer_islands(dtype, src, S, ld_src, n, starts, I, members, slots, master, mom, K_state,
                                     ld_state, first, lr, momentum, dampening, wd, nesterov, x, ld_x, None)


@pytest.mark.parametrize("bad", [
    dict(n=-1), dict(S=0), dict(S=-3), dict(K_state=0), dict(K_state=-1), dict(I=0), dict(I=-1), dict(I=65536),
    dict(src=None), dict(master=None), dict(x=None), dict(starts=None), dict(members=None), dict(slots=None),
    dict(mom=None), dict(ld_src=N - 1), dict(ld_x=N - 1), dict(ld_state=N - 1),
    dict(master=ctypes.c_void_p(66)), dict(mom=ctypes.c_void_p(65)),
    dict(dampening=0.1), dict(momentum=0.0, mom=None), dict(momentum=-0.5), dict(dtype=7), dict(dtype=2),
])
def test_invalid_arguments_fail_cleanly(bad):
    L = _lib()
    assert _islands(L, **bad) == 1  # GA_EINVAL, checked on the host before any launch
    assert NAME in L.ga_last_error().decode()


def test_zero_length_is_a_noop():
    L = _lib()
    assert _islands(L, n=0, src=None, master=None, mom=None, x=None, starts=None, members=None, slots=None) == 0
    assert L.ga_last_error().decode() == ""
    assert _islands(L, n=0, I=0) == 1 and _islands(L, n=0, S=0) == 1  # ...but not a licence for bad sizes


def test_ops_refuse_cpu_tensors():
    import torch
    from gym_amd import ops
    x, m = torch.zeros(2, N), torch.zeros(2, N)
    args = (N, 0.7, 0.0, 0.0, 0.0, False, True)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.diloco_outer_islands(x, [[0, 1]], [[0, 1]], m, None, x, *args)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.diloco_outer_islands(torch.zeros(3, N), [[0, 2]], [[-1, 0]], m[:1], None, x[:1], *args)


@pytest.mark.parametrize("islands,slots,match", [
    ([], [], "0 islands"),
    ([[0, 1]], [[0, 1], [2]], "1 islands with 2 slot lists"),
    ([[0, 1], []], [[0, 1], []], "island 1 is empty"),
    ([[0, 1]], [[0]], "2 members and 1 slots"),
    ([[1, 0]], [[0, 1]], "not ascending"),
    ([[0, 0]], [[0, 1]], "not ascending"),
    ([[0, 3]], [[0, 1]], "outside"),
    ([[-1, 0]], [[0, 1]], "outside"),
    ([[0, 1]], [[0, 2]], "slot 2"),
    ([[0, 1]], [[-2, 0]], "slot -2"),
    ([[0], [1, 2]], [[1], [0, 1]], "used twice"),
    ([[0, 1], [2]], [[-1, -1], [-1]], "no slot >= 0"),
])
def test_ops_refuse_malformed_host_tables(islands, slots, match):
    """S = 3 source rows, K_state = 2 state rows; refused on the host, before the GPU check."""
    import torch
    from gym_amd import ops
    x, m = torch.zeros(2, N), torch.zeros(2, N)
    with pytest.raises(ValueError, match=match):
        ops.diloco_outer_islands(torch.zeros(3, N), islands, slots, m, None, x, N, 0.7, 0.0, 0.0, 0.0, False, True)
    with pytest.raises(ValueError, match=match):
        ops.island_table(islands, slots, 3, 2)


def test_host_table_layout():
    from gym_amd import ops
    assert ops.island_table([[0, 3], [1, 2, 4]], [[0, -1], [1, 2, 4]], 5, 5) == [0, 2, 5, 0, 3, 1, 2, 4, 0, -1, 1, 2, 4]
    assert ops.island_table([[2]], [[0]], 3, 1) == [0, 1, 2, 0]
