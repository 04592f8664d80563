"""8-bit AdamW without a GPU: the "adamw8bit" spec, the code books, the torch class against
the numpy restatement (adam8_checks), its state dict, and the host argument checks of
ga_adam8_step / ga_adam8_encode."""
import ctypes

import numpy as np
import pytest
import torch

import adam8_checks as A


def test_spec_name_builds_the_torch_class():
    from gym_amd.strategy.optim import AdamW8bit, OptimSpec
    opt = OptimSpec.from_string("adamw8bit", lr=3e-3, betas=(0.8, 0.9)).build([torch.nn.Parameter(torch.zeros(3))])
    assert type(opt) is AdamW8bit and opt.param_groups[0]["lr"] == 3e-3 and opt.param_groups[0]["betas"] == (0.8, 0.9)


def test_tables():
    codes, thr = A.tables()
    assert codes.dtype == thr.dtype == np.float32 and codes.shape == thr.shape == (2, 256)
    for r in range(2):
        assert len(set(codes[r])) == 256 and (np.diff(codes[r]) > 0).all()
        assert len(set(thr[r, :255])) == 255
        assert ((thr[r, :255] > codes[r, :-1]) & (thr[r, :255] < codes[r, 1:])).all()
    assert codes[0, 127] == 0 and codes[1, 0] == 0
    assert codes[1, 1] == np.float32(3.25e-7)
    assert codes[0, 0] == np.float32(-0.99296874) and codes[0, 255] == 1 and codes[1, 255] == 1


def _toy(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in [(5, 7), (130,), (64, 3)]]


def _grads(ps, t):
    g = torch.Generator().manual_seed(100 + t)
    for i, p in enumerate(ps):
        p.grad = torch.randn(p.shape, generator=g) * 10.0 ** (i - 1)


def test_torch_class_equals_the_restatement():
    from gym_amd.strategy.optim import AdamW8bit
    ps = _toy()
    want = [p.detach().numpy().reshape(-1).copy() for p in ps]
    states = [None] * len(ps)
    opt = AdamW8bit(ps, lr=1e-2, weight_decay=0.1)
    for t in range(1, 4):
        _grads(ps, t)
        opt.step()
        for i, p in enumerate(ps):
            n, nb = p.numel(), -(-p.numel() // 64) * 64
            x, g = np.zeros(nb, np.float32), np.zeros(nb, np.float32)
            x[:n], g[:n] = want[i], p.grad.numpy().reshape(-1)
            x, _, states[i] = A.step(x, g, states[i] or A.fresh(nb), t, lr=1e-2, weight_decay=0.1)
            want[i] = x[:n]
            st = opt.state[p]
            assert float(st["step"]) == t and np.array_equal(p.detach().numpy().reshape(-1), want[i])
            for key, w in zip(("exp_avg_code", "exp_avg_absmax", "exp_avg_sq_code", "exp_avg_sq_absmax"), states[i]):
                assert st[key].numpy().dtype == w.dtype and np.array_equal(st[key].numpy(), w), (t, i, key)


def test_state_dict_round_trip():
    from gym_amd.strategy.optim import AdamW8bit
    a, b = _toy(), _toy()
    oa, ob = AdamW8bit(a, lr=1e-2), AdamW8bit(b, lr=1e-2)
    for t in range(1, 3):
        _grads(a, t)
        oa.step()
    with torch.no_grad():
        for p, q in zip(a, b):
            q.copy_(p)
    ob.load_state_dict(oa.state_dict())
    assert ob.state[b[0]]["exp_avg_code"].dtype == torch.uint8 and float(ob.state[b[0]]["step"]) == 2
    for ps, o in ((a, oa), (b, ob)):
        _grads(ps, 3)
        o.step()
    for p, q in zip(a, b):
        assert torch.equal(p, q)
        assert all(torch.equal(oa.state[p][k], ob.state[q][k]) for k in oa.state[p])


_HP = (0.1, 0.999, 0.001, 1e-8, 1.0, 0.0, -1e-3, 0.5)


def _step(L, a, dtype=0, p=256, g=256, mc=64, ma=64, vc=64, va=64, K=1, ld=64, n=64, codes=64, thr=64, hp=_HP):
    return L.ga_adam8_step(dtype, a(p), a(g), a(mc), a(ma), a(vc), a(va), K, ld, n, a(codes), a(thr), *hp, None, None)


def _encode(L, a, x=256, code=64, absmax=64, K=1, ld=64, n=64, row=0, thr=64):
    return L.ga_adam8_encode(a(x), a(code), a(absmax), K, ld, n, row, a(thr), None)


@pytest.mark.parametrize("fn,kw,msg", [
    (_step, dict(p=None), "null"), (_step, dict(va=None), "null"), (_step, dict(thr=None), "null"),
    (_step, dict(g=264), "16-byte"), (_step, dict(mc=66), "4-byte"), (_step, dict(vc=65), "4-byte"),
    (_step, dict(ld=96, n=64, K=2), "ld"), (_step, dict(ld=64, n=128, K=2), "ld"), (_step, dict(n=32), "n must"),
    (_step, dict(hp=_HP[:7] + (0.0,)), "bc2_sqrt"), (_step, dict(dtype=1), "float32"), (_step, dict(K=0), "sizes"),
    (_encode, dict(code=None), "null"), (_encode, dict(x=260), "16-byte"), (_encode, dict(code=66), "4-byte"),
    (_encode, dict(ld=96), "ld"), (_encode, dict(n=100, ld=128), "n must"), (_encode, dict(row=2), "row"),
    (_encode, dict(K=70000), "sizes"),
])
def test_invalid_arguments_fail_cleanly(fn, kw, msg):
    """Checked on the host before any launch: GA_EINVAL and the entry's name in the message."""
    from gym_amd import _lib
    L = _lib.lib()
    assert fn(L, ctypes.c_void_p, **kw) == 1
    err = L.ga_last_error().decode()
    assert msg in err and err.startswith("ga_adam8_step" if fn is _step else "ga_adam8_encode")


def test_zero_length_is_a_noop():
    from gym_amd import _lib
    L = _lib.lib()
    none = lambda _: None  # noqa: E731
    assert _step(L, none, n=0, ld=0) == 0 and L.ga_last_error().decode() == ""
    assert _encode(L, none, n=0, ld=0) == 0 and L.ga_last_error().decode() == ""
