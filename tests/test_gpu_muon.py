"""The fused Muon inner step (ArenaMuon through build_fused: ga_muon_prepare / scale / gemm /
apply and the inner ArenaAdam) against a float64 restatement of torch.optim.Muon without any
bf16 rounding, on an arena of Muon matrices with other tensors between them.

Shapes, by the boundary they hit (macro tile 128, or 64 when the short side is <= 64; k-step 64;
prepare / apply tiles 64 x 64):
  10 x 128, 128 x 10   below one MFMA tile in m, flat and tall (64-tile class, 2 k-steps)
  33 x 47              ragged in both dimensions, one 64 tile
  48 x 200             64-tile class, 4 k-steps of the gram and 4 column tiles of the update
  200 x 65             tall and ragged, m = 65 just past the 64-tile class (128-tile class)
  96 x 96              square, one 128 tile
  160 x 416            2 x 4 macro tiles (an off-diagonal symmetric tile and its mirror), 8 / 4 k-steps

ns_steps >= 1: e = |O - O_f64|_F / |O_f64|_F per matrix is held to 2 e_ref, e_ref the same error
of torch's own _zeropower_via_newtonschulz in bf16 on the CPU, the maximum over this case's inputs
of that shape (steps and replicas).

ns_steps = 0: the issue's bar, 2^-8 per element plus 2^-8 for the norm (2^-7 |O_f64| together), is
held with one addition: an absolute term 3 * 2^-24 * max|p| / adjusted_lr (about 1e-8 against |O| of
about 1e-2).  O is not an output of the step; the test recovers it as (p (1 - lr wd) - p_new) /
adjusted_lr from fp32 parameters, and that term is the fp32 rounding of the three operations involved,
which an element of O near zero would otherwise be charged with."""
import numpy as np
import pytest
import torch
from torch.optim._muon import _zeropower_via_newtonschulz

import optim_cases as S

pytestmark = pytest.mark.gpu

SHAPES = [(10, 128), (7,), (128, 10), (33, 47), (5, 3), (48, 200), (200, 65), (13,), (96, 96), (160, 416), (70,)]
MASK = [len(s) == 2 and s != (5, 3) for s in SHAPES]
ABSENT = 3  # the 33 x 47 matrix
COEF = (3.4445, -4.775, 2.0315)
HP = dict(lr=0.5, weight_decay=0.1, momentum=0.9, eps=1e-7, adamw_lr=1e-2, adamw_weight_decay=0.05)
SLACK = 64


class Bag(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=g) * 0.02) for s in SHAPES])


def _grads(seed, step, k):
    """Full-rank Gaussian on the first step, heavy-tailed (1% of the entries x 100) on the second."""
    rng = np.random.default_rng([seed, step, k])
    out = []
    for s in SHAPES:
        g = rng.standard_normal(s) * 1e-2
        if step % 2:
            g = np.where(rng.random(s) < 0.01, 100.0 * g, g)
        out.append(g.astype(np.float32))
    return out


def _ns64(u, ns):
    x = u.T if u.shape[0] > u.shape[1] else u
    x = x / max(np.linalg.norm(x), HP["eps"])
    a, b, c = COEF
    for _ in range(ns):
        A = x @ x.T
        x = a * x + (b * A + c * A @ A) @ x
    return x.T if u.shape[0] > u.shape[1] else x


def _setup(ns, nesterov, K):
    """K replicas of the bag in a ReplicaArena whose parameter set has 64 sentinel elements
    behind the last row, and the fused optimizer build_fused gives for the spec."""
    from gym_amd.arena import ReplicaArena
    from gym_amd.fused_optim import ArenaMuon, build_fused
    from gym_amd.strategy.optim import MuonAdamW, OptimSpec
    dev = torch.device("cuda:0")
    models = [Bag(5).to(dev) for _ in range(K)]
    ra = ReplicaArena(models)
    big = torch.full((K * ra.ld + SLACK,), 7.0, device=dev)
    big[:K * ra.ld] = 0
    ra.relocate_params(big[:K * ra.ld].view(K, ra.ld))
    spec = OptimSpec(MuonAdamW, muon_mask=MASK, ns_steps=ns, nesterov=nesterov, **HP)  # fused by default
    opt = build_fused(spec, ra.params, ra, models=models)
    assert isinstance(opt, ArenaMuon)
    return models, ra, big, opt


def _step(models, ra, opt, t, grad_rows, max_norm, gone):
    """Step t: replica k takes the gradients of grad_rows[k]; gone: the ABSENT matrix has none."""
    ra.zero_grad()
    for k, m in enumerate(models):
        for i, (p, g) in enumerate(zip(m.parameters(), _grads(11, t, grad_rows[k]))):
            if gone and i == ABSENT:
                p.grad = None
            else:
                p.grad.copy_(torch.from_numpy(g))
    opt.step(max_norm=max_norm)


def _run(ns, nesterov, K, max_norm, absent, grad_rows=None):
    """Two steps of the fused optimizer.  Returns the setup and, per step, (parameters before,
    after, momentum buffers after) as [K][tensor] arrays, and the raw flat buffers before / after."""
    models, ra, big, opt = _setup(ns, nesterov, K)
    host = lambda m: [p.detach().cpu().numpy().copy() for p in m.parameters()]  # noqa: E731
    steps, raw = [], [big.cpu().numpy().copy()]
    for t in range(2):
        before = [host(m) for m in models]
        _step(models, ra, opt, t, grad_rows or list(range(K)), max_norm, absent and t == 1)
        bufs = [[opt.state[p]["momentum_buffer"].cpu().numpy().copy() if MASK[i] else None
                 for i, p in enumerate(m.parameters())] for m in models]
        steps.append((before, [host(m) for m in models], bufs))
    raw.append(big.cpu().numpy().copy())
    return (models, ra, opt), steps, raw


CASES = [  # ns_steps, nesterov, K, max_norm, a Muon matrix absent on the second step
    (0, True, 1, None, False), (0, False, 3, 0.05, False), (1, False, 1, None, False), (1, True, 1, None, True),
    (5, True, 1, None, False), (5, True, 3, 0.05, False)]


@pytest.mark.parametrize("ns,nesterov,K,max_norm,absent", CASES)
def test_fused_muon_step(ns, nesterov, K, max_norm, absent):
    (models, ra, opt), steps, raw = _run(ns, nesterov, K, max_norm, absent)
    lr, wd, mom = HP["lr"], HP["weight_decay"], HP["momentum"]
    layout = ra.layout
    errs = {}  # matrix index -> [(e, e_ref)] over steps and replicas
    for k in range(K):
        buf = [np.zeros(s) for s in SHAPES]
        ref = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p, m in zip(steps[0][0][k], MASK) if not m]
        adamw = torch.optim.AdamW(ref, lr=HP["adamw_lr"], weight_decay=HP["adamw_weight_decay"])
        for t, (before, after, bufs) in enumerate(steps):
            g32 = _grads(11, t, k)
            gone = absent and t == 1
            norm = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for i, g in enumerate(g32)
                               if not (gone and i == ABSENT)))
            coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm else 1.0
            for i, s in enumerate(SHAPES):
                if not MASK[i]:
                    continue
                p0, p1 = before[k][i].astype(np.float64), after[k][i].astype(np.float64)
                if gone and i == ABSENT:  # skipped exactly: no decay, no buffer change
                    assert np.array_equal(before[k][i], after[k][i]) and np.array_equal(bufs[k][i], steps[0][2][k][i])
                    continue
                g = g32[i].astype(np.float64) * coef
                buf[i] = buf[i] + (1 - mom) * (g - buf[i])
                np.testing.assert_allclose(bufs[k][i], buf[i], rtol=1e-5, atol=1e-7)
                u = g + mom * (buf[i] - g) if nesterov else buf[i]
                adj = lr * np.sqrt(max(1.0, s[0] / s[1]))
                O = (p0 * (1 - lr * wd) - p1) / adj
                want = _ns64(u, ns)
                if ns == 0:
                    # one bf16 rounding of u (2^-9, half an ulp; 2^-8 allowed) plus 2^-8 for the norm; O is
                    # recovered from fp32 parameters: three roundings at the size of p, divided by adjusted_lr
                    slack = 3 * 2.0 ** -24 * max(np.abs(p0).max(), np.abs(p1).max()) / adj
                    assert (np.abs(O - want) <= 2.0 ** -7 * np.abs(want) + slack).all(), (s, np.abs(O - want).max())
                else:
                    tor = _zeropower_via_newtonschulz(torch.from_numpy(u.astype(np.float32)), COEF, ns, HP["eps"])
                    den = np.linalg.norm(want)
                    errs.setdefault(i, []).append((np.linalg.norm(O - want) / den,
                                                   np.linalg.norm(tor.double().numpy() - want) / den))
            for p, i in zip(ref, [i for i, m in enumerate(MASK) if not m]):
                p.grad = torch.from_numpy((g32[i].astype(np.float64) * coef).astype(np.float32))
            adamw.step()
            S.assert_close([after[k][i] for i, m in enumerate(MASK) if not m], [p.detach().numpy() for p in ref])
    for i, pairs in errs.items():
        e, e_ref = max(p[0] for p in pairs), max(p[1] for p in pairs)
        print(f"muon {SHAPES[i]} ns={ns}: e={e:.4g} e_ref={e_ref:.4g} ratio={e / e_ref:.3f}")
        assert e <= 2 * e_ref, (SHAPES[i], ns, e, e_ref)
    # untouched: the arena padding of every row and the 64 elements behind the last row
    pad = np.ones(ra.ld, bool)
    for o, n in zip(layout.offsets, layout.numels):
        pad[o:o + n] = False
    pad = np.concatenate([np.tile(pad, K), np.ones(SLACK, bool)])
    assert np.array_equal(raw[0][pad], raw[1][pad]) and (raw[1][-SLACK:] == 7.0).all()
    Bpad = opt.B.cpu().numpy().reshape(-1)
    owned = np.zeros(ra.ld, bool)
    for (o, n), m in zip(zip(layout.offsets, layout.numels), MASK):
        owned[o:o + n] = m
    assert not Bpad[np.tile(~owned, K)].any()
    if K == 1 and ns == 5:  # determinism: no atomics anywhere, the same bits twice
        again = _run(ns, nesterov, K, max_norm, absent)[2][1]
        assert np.array_equal(raw[1], again)
    for k in range(K if K > 1 else 0):  # every replica equals its own K = 1 run, bitwise
        alone = _run(ns, nesterov, 1, max_norm, absent, grad_rows=[k])[1][1][1][0]
        for a, b in zip(steps[1][1][k], alone):
            assert np.array_equal(a, b), k
    # state_dict -> a fresh ArenaMuon -> load_state_dict -> an identical third step, state still in the flat buffers
    models2, ra2, _, opt2 = _setup(ns, nesterov, K)
    ra2.flat_set.copy_(ra.flat_set)
    opt2.load_state_dict(opt.state_dict())
    for ms, r, o in ((models, ra, opt), (models2, ra2, opt2)):
        _step(ms, r, o, 2, list(range(K)), max_norm, False)
    assert torch.equal(ra.flat_set, ra2.flat_set) and torch.equal(opt.B, opt2.B)
    assert torch.equal(opt.adam.M, opt2.adam.M) and torch.equal(opt.adam.V, opt2.adam.V)
    for p, flat in ((models2[-1].ps[0], opt2.B), (models2[-1].ps[1], opt2.adam.M)):
        st = opt2.state[p]["momentum_buffer" if flat is opt2.B else "exp_avg"]
        assert st.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
    assert [float(opt2.state[p]["step"]) for p in models2[0].ps if "step" in opt2.state[p]] == [3.0] * MASK.count(False)


def _strategy():
    from gym_amd.strategy import DiLoCoStrategy, OptimSpec
    return DiLoCoStrategy(optim_spec=OptimSpec.from_string("muon", lr=0.02), H=2)


def _fit(replicas, port):
    from tiny_models import TinyMLP, dataset
    from gym_amd.trainer import LocalTrainer
    torch.manual_seed(0)
    tr = LocalTrainer(TinyMLP(), dataset(256), dataset(64, seed=1), start_port=port)
    strategy = _strategy()
    tr.fit(num_epochs=1, strategy=strategy, num_nodes=2, max_steps=4, devices=[0], batch_size=16, minibatch_size=16,
           val_size=16, val_interval=100, replicas_per_process=replicas, keep_node_states=True)
    return tr.node_states


def test_muon_spec_is_fused_in_both_modes_and_reports_its_selection(monkeypatch):
    """What fit builds for _strategy(): ArenaMuon in process mode (_init_node) and in replica mode
    (ReplicaRunner), MuonAdamW under GA_FUSED_OPTIM=0, and the selected matrices in __config__()
    every time."""
    from tiny_models import TinyMLP
    from gym_amd.fused_optim import ArenaMuon
    from gym_amd.replica import ReplicaRunner
    from gym_amd.strategy.optim import MuonAdamW
    dev = torch.device("cuda:0")
    names = [n for n, p in TinyMLP().named_parameters() if p.ndim == 2]
    assert names
    for fused in (True, False):
        monkeypatch.setenv("GA_FUSED_OPTIM", "1" if fused else "0")
        s = _strategy()
        s._init_node(TinyMLP().to(dev), 0, 1)
        assert type(s.optim) is (ArenaMuon if fused else MuonAdamW)
        assert s.__config__()["muon_matrices"] == names
        s = _strategy()
        runner = ReplicaRunner(s, [TinyMLP().to(dev) for _ in range(2)], rank=0, num_nodes=2)
        assert type(runner.optim) is ArenaMuon if fused else type(runner.optim.opts[0]) is MuonAdamW
        assert s.__config__()["muon_matrices"] == names


def test_diloco_muon_trainer_fit_both_modes():
    """DiLoCoStrategy(optim_spec="muon") through LocalTrainer.fit: both nodes in one process against
    one process per node.  The replica pass is the process pass (one workspace, the same tables),
    so the modes agree far inside the 2 e_ref bar: held to assert_close."""
    rep, proc = _fit(2, 22700), _fit(1, 22720)
    for r in range(2):
        for name in rep[r]:
            assert torch.isfinite(rep[r][name]).all()
            np.testing.assert_allclose(rep[r][name].cpu().numpy(), proc[r][name].cpu().numpy(), rtol=1e-4, atol=1e-6)
