"""Fused SGD inner optimizer (ArenaSGD) host logic on CPU, with the kernel
stand-ins of tests/fake_sgd_ops.py, against torch.optim.SGD and
clip_grad_norm_: presence patterns, `first` flags, launches, state dicts,
constructor errors, fusable_sgd, the strategies' wiring and ga_sgd_step's host
argument checks."""
import copy
import ctypes

import pytest
import torch

import sgd_cases as S


@pytest.fixture
def fake(monkeypatch):
    import fake_sgd_ops
    import gym_amd.fused_optim as fo
    monkeypatch.setattr(fo, "ops", fake_sgd_ops)
    return fake_sgd_ops


def absent_spans_unchanged(snap):
    """An observer for sgd_cases.run_pair: over every step on which a parameter is
    absent (or frozen), its value and its span of the momentum buffer stay
    bit-identical."""
    def spans(ctx, step):
        opt = ctx["opt"]
        for k, (m, pat) in enumerate(zip(ctx["models"], ctx["pats"])):
            for i, p in enumerate(m.parameters()):
                if not pat.present(i, step):
                    _, o, n = opt._where[id(p)]
                    cur = [p.detach().clone()]
                    if opt.B is not None:
                        cur.append(opt.B[k, o:o + n].clone())
                    yield (k, i), cur

    def observe(when, step, ctx):
        for key, cur in spans(ctx, step):
            if when == "before":
                snap[key] = cur
            else:
                for name, x, y in zip(("param", "momentum_buffer"), snap.pop(key), cur):
                    assert torch.equal(x, y), f"step {step} replica/tensor {key}: absent, but its {name} moved"
    return observe


@pytest.mark.parametrize("name,kw,max_norm,pattern", S.CASES, ids=[c[0] for c in S.CASES])
def test_arena_sgd_host_logic(fake, name, kw, max_norm, pattern):
    ours, ref = S.run_pair("cpu", kw, max_norm=max_norm, pattern=pattern, observe=absent_spans_unchanged({}))
    S.assert_same(ours, ref)


@pytest.mark.parametrize("name,kw,max_norm", S.REPLICA_CASES, ids=[c[0] for c in S.REPLICA_CASES])
def test_arena_sgd_replicas_host_logic(fake, name, kw, max_norm):
    """K = 3 rows of a ReplicaArena, a different presence pattern on each, against
    three independent torch optimizers."""
    ours, ref = S.run_pair("cpu", kw, max_norm=max_norm, pattern=S.REPLICA_PATTERNS, K=3,
                           observe=absent_spans_unchanged({}))
    S.assert_same(ours, ref)


def _record_launches(fake, monkeypatch):
    """Wrap the stand-in's sgd_step: calls[i] = (param, buf, first, clip buffer)."""
    calls, real = [], fake.sgd_step

    def sgd_step(param, grad, buf, **kw):
        calls.append((param, buf, kw["first"], kw.get("clip_coef")))
        return real(param, grad, buf, **kw)

    monkeypatch.setattr(fake, "sgd_step", sgd_step)
    return calls


def test_all_present_is_one_launch_over_the_whole_set(fake, monkeypatch):
    """Every parameter present on every step: one sgd_step call per step over the
    full [K, ld] sets with the clip buffer whole; first=1 on the first step and 0
    afterwards.  K = 1 and K = 3."""
    calls = _record_launches(fake, monkeypatch)
    for K in (1, 3):
        seen = {}

        def observe(when, step, ctx):
            if when == "before":
                seen["n"] = len(calls)
                return
            opt = ctx["opt"]
            assert len(calls) == seen["n"] + 1, f"step {step}: {len(calls) - seen['n']} launches"
            param, buf, first, clip = calls[-1]
            assert param.data_ptr() == opt.P.data_ptr() and tuple(param.shape) == (K, opt.ld)
            assert buf.data_ptr() == opt.B.data_ptr() and tuple(buf.shape) == (K, opt.ld)
            assert clip.data_ptr() == opt._clip.data_ptr() and clip.numel() == 2 * K
            assert bool(first) == (step == 0)

        ours, ref = S.run_pair("cpu", {"lr": 0.1, "momentum": 0.9}, max_norm=0.5, pattern=[S.Pattern()] * K, K=K,
                               steps=4, observe=observe)
        S.assert_same(ours, ref)


def test_no_momentum_passes_no_buffer_and_keeps_no_state(fake, monkeypatch):
    calls = _record_launches(fake, monkeypatch)
    states = []

    def observe(when, step, ctx):
        if when == "after":
            states.append((len(ctx["opt"].state), ctx["opt"].B))

    ours, ref = S.run_pair("cpu", {"lr": 0.1, "weight_decay": 0.05}, steps=3, observe=observe)
    S.assert_same(ours, ref)
    assert len(calls) == 3 and all(buf is None and not first for _, buf, first, _ in calls)
    assert states == [(0, None)] * 3
    assert ours["has_buffer"] == [False] * len(S.SHAPES)


def test_late_start_gets_its_own_first_launch(fake, monkeypatch):
    """Tensor 1 absent at steps 0-1 (optim_cases "late-start"): (a, b, first) of
    every launch.  Tensor offsets 0, 2112, 2240, 8384, 8448; the last tensor ends
    at 8458; ld 8704.  At step 2 tensor 1 takes first=1 between two first=0
    ranges; from step 3 on the row is one launch again."""
    calls = _record_launches(fake, monkeypatch)
    got, has = [], []

    def observe(when, step, ctx):
        if when == "after":
            flat = ctx["arena"].flat
            for param, _, first, _ in calls:
                a = (param.data_ptr() - flat.data_ptr()) // 4
                got.append((step, a, a + param.numel(), bool(first)))
            calls.clear()
            opt = ctx["opt"]
            has.append([opt.state[p]["momentum_buffer"] is not None for p in ctx["models"][0].parameters()])

    ours, ref = S.run_pair("cpu", {"lr": 0.1, "momentum": 0.9}, pattern=dict(S.PATTERNS)["late-start"], steps=4,
                           observe=observe)
    S.assert_same(ours, ref)
    n = 8704
    assert got == [(0, 0, 2112, True), (0, 2240, 8458, True),
                   (1, 0, 2112, False), (1, 2240, 8458, False),
                   (2, 0, 2112, False), (2, 2112, 2240, True), (2, 2240, 8458, False),
                   (3, 0, n, False)]
    assert has == [[True, False, True, True, True]] * 2 + [[True] * 5] * 2


def test_step_without_any_gradient_launches_nothing(fake, monkeypatch):
    calls = _record_launches(fake, monkeypatch)
    per_step = []

    def observe(when, step, ctx):
        if when == "after":
            per_step.append(len(calls))
            calls.clear()

    ours, ref = S.run_pair("cpu", {"lr": 0.1, "momentum": 0.9}, max_norm=0.5, pattern=dict(S.PATTERNS)["empty-step"],
                           steps=4, observe=observe)
    S.assert_same(ours, ref)
    assert per_step == [1, 1, 0, 1]


_PAT = S.Pattern({1: (0, 1), 3: (0, 1, 2, 3)})  # tensor 1 late, tensor 3 without a gradient before the save


def _drive(model, opt, steps, arena=None):
    for step in steps:
        if arena is not None:
            arena.zero_grad()
        for i, (p, g) in enumerate(zip(model.parameters(), S.grads_for(step))):
            p.grad = g.clone() if _PAT.present(i, step) else None
        if arena is not None:
            opt.step(max_norm=0.5)
        else:
            torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.grad is not None], 0.5)
            opt.step()


@pytest.mark.parametrize("source", ["arena", "torch"])
def test_state_dict_round_trip_continues_the_run(fake, source):
    """Two steps (tensor 1 and tensor 3 still without a buffer: torch has no entry
    / a None buffer for them), save, load into a fresh ArenaSGD, four more steps
    (tensor 1 starts at step 2, tensor 3 at step 4: each with its own first
    launch) == the uninterrupted torch run."""
    from gym_amd.arena import ParamArena
    from gym_amd.fused_optim import ArenaSGD
    kw = {"lr": 0.1, "momentum": 0.9, "dampening": 0.1, "weight_decay": 0.05}
    tm, am = S.make_model("cpu"), S.make_model("cpu")
    arena = ParamArena(list(am.parameters()))
    topt, aopt = torch.optim.SGD(tm.parameters(), **kw), ArenaSGD(am.parameters(), arena, **kw)
    _drive(tm, topt, range(2))
    _drive(am, aopt, range(2), arena)
    if source == "torch":
        saved, params = copy.deepcopy(topt.state_dict()), list(tm.parameters())
        saved["state"][3] = {"momentum_buffer": None}  # what torch saves for a parameter it skipped: nothing, or None
        assert 1 not in saved["state"]
    else:
        saved, params = copy.deepcopy(aopt.state_dict()), list(am.parameters())
        assert saved["state"][1]["momentum_buffer"] is None and saved["state"][0]["momentum_buffer"] is not None
        assert set(saved["param_groups"][0]) == set(topt.state_dict()["param_groups"][0])
    bm = S.make_model("cpu", seed=99)
    with torch.no_grad():
        for p, q in zip(bm.parameters(), params):
            p.copy_(q)
    barena = ParamArena(list(bm.parameters()))
    bopt = ArenaSGD(bm.parameters(), barena, lr=0.5)  # the loaded group replaces these settings
    bopt.load_state_dict(saved)
    assert S._state(bopt, list(bm.parameters()))["has_buffer"] == [True, False, True, False, True]
    assert bopt.state[next(bm.parameters())]["momentum_buffer"].data_ptr() == bopt.B.data_ptr()
    _drive(bm, bopt, range(2, 6), barena)
    _drive(tm, topt, range(2, 6))
    S.assert_same(S._state(bopt, list(bm.parameters())), S._state(topt, list(tm.parameters())))


def test_arena_state_dict_loads_into_torch_sgd(fake):
    """The other direction: an ArenaSGD state dict (None buffers included) resumes
    in torch.optim.SGD."""
    from gym_amd.arena import ParamArena
    from gym_amd.fused_optim import ArenaSGD
    kw = {"lr": 0.1, "momentum": 0.9}
    tm, am = S.make_model("cpu"), S.make_model("cpu")
    arena = ParamArena(list(am.parameters()))
    topt, aopt = torch.optim.SGD(tm.parameters(), **kw), ArenaSGD(am.parameters(), arena, **kw)
    _drive(tm, topt, range(2))
    _drive(am, aopt, range(2), arena)
    bm = S.make_model("cpu", seed=99)
    with torch.no_grad():
        for p, q in zip(bm.parameters(), am.parameters()):
            p.copy_(q)
    bopt = torch.optim.SGD(bm.parameters(), **kw)
    bopt.load_state_dict(copy.deepcopy(aopt.state_dict()))
    _drive(bm, bopt, range(2, 6))
    _drive(tm, topt, range(2, 6))
    S.assert_same(S._state(bopt, list(bm.parameters())), S._state(topt, list(tm.parameters())))


@pytest.mark.parametrize("kw", [{"lr": -0.1}, {"momentum": -0.5}, {"weight_decay": -1e-3},
                                {"nesterov": True}, {"nesterov": True, "momentum": 0.9, "dampening": 0.1}],
                         ids=["lr", "momentum", "weight_decay", "nesterov-no-momentum", "nesterov-dampening"])
def test_constructor_errors_are_torchs(fake, kw):
    from gym_amd.arena import ParamArena
    from gym_amd.fused_optim import ArenaSGD
    m = S.make_model("cpu")
    with pytest.raises(ValueError) as theirs:
        torch.optim.SGD(m.parameters(), **kw)
    with pytest.raises(ValueError) as ours:
        ArenaSGD(m.parameters(), ParamArena(list(m.parameters())), **kw)
    assert str(ours.value) == str(theirs.value)


def test_constructor_needs_one_group_inside_the_arena(fake):
    from gym_amd.arena import ParamArena
    from gym_amd.fused_optim import ArenaSGD
    m = S.make_model("cpu")
    ps = list(m.parameters())
    arena = ParamArena(ps)
    with pytest.raises(ValueError, match="one parameter group"):
        ArenaSGD([{"params": ps[:2]}, {"params": ps[2:]}], arena)
    with pytest.raises(ValueError, match="must live in the arena"):
        ArenaSGD(ps + [torch.nn.Parameter(torch.zeros(3))], arena)
    opt = ArenaSGD(ps, arena, lr=0.1, momentum=0.9, placement=True)
    assert opt.placement == {"placed": False, "why": "no search for SGD"}
    assert opt.param_groups[0]["lr"] == 0.1 and set(opt.param_groups[0]) == set(
        torch.optim.SGD(S.make_model("cpu").parameters(), lr=0.1).param_groups[0])


def test_fusable_sgd_truth_table():
    from gym_amd.arena import ParamArena
    from gym_amd.fused_optim import fusable, fusable_sgd
    SGD = torch.optim.SGD
    arena = ParamArena(list(S.make_model("cpu").parameters()))
    nograd = ParamArena(list(S.make_model("cpu").parameters()), with_grad=False)
    bf16 = ParamArena(list(S.make_model("cpu").to(torch.bfloat16).parameters()))
    yes = [{}, {"lr": 0.1}, {"lr": 0.1, "momentum": 0.9, "dampening": 0.1, "weight_decay": 1e-4},
           {"momentum": 0.9, "nesterov": True}, {"foreach": True}, {"fused": False}, {"maximize": False},
           {"differentiable": False}]
    no = [{"maximize": True}, {"differentiable": True}, {"lr": torch.tensor(0.1)}, {"unknown_option": 1}]
    for kw in yes:
        assert fusable_sgd(SGD, kw, arena), kw
    for kw in no:
        assert not fusable_sgd(SGD, kw, arena), kw
    assert fusable_sgd(SGD, None, arena)
    assert not fusable_sgd(SGD, {}, None) and not fusable_sgd(SGD, {}, nograd) and not fusable_sgd(SGD, {}, bf16)
    for cls in (torch.optim.AdamW, torch.optim.Adam, torch.optim.RMSprop):
        assert not fusable_sgd(cls, {}, arena)
    # fusable() keeps its meaning: Adam / AdamW only
    assert fusable(torch.optim.AdamW, {}, arena) and not fusable(SGD, {"lr": 0.1}, arena)


def _built(monkeypatch, spec, replica):
    """The inner optimizer a strategy ends up with, process-per-node or replica mode."""
    import fake_sgd_ops
    import gym_amd.strategy.strategy as strategy
    from gym_amd.strategy import SimpleReduceStrategy
    monkeypatch.setattr(strategy, "require_gpu", lambda device: None)
    for name in ("gym_amd.engine", "gym_amd.fused_optim", "gym_amd.replica"):
        monkeypatch.setattr(__import__(name, fromlist=["ops"]), "ops", fake_sgd_ops)
    s = SimpleReduceStrategy(optim_spec=spec, max_norm=0.5)
    if replica:
        from gym_amd.replica import ReplicaRunner
        runner = ReplicaRunner(s, [S.make_model("cpu") for _ in range(2)], rank=0, num_nodes=2)
        return runner, runner.optim
    s._init_node(S.make_model("cpu"), 0, 1)
    return s, s.optim


@pytest.mark.parametrize("replica", [False, True], ids=["process", "replica"])
def test_strategies_build_arena_sgd(monkeypatch, replica):
    """OptimSpec(torch.optim.SGD, ...) (and the reference's "sgd" string) becomes an
    ArenaSGD in both modes and steps through it; GA_FUSED_OPTIM=0 keeps torch's SGD."""
    from gym_amd.strategy import OptimSpec
    spec = OptimSpec(torch.optim.SGD, lr=0.1, momentum=0.9)
    owner, opt = _built(monkeypatch, spec, replica)
    assert type(opt).__name__ == "ArenaSGD"
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["nesterov"]) == (0.1, 0.9, False)
    before = [p.detach().clone() for p in opt.param_groups[0]["params"]]
    owner.zero_grad()
    for p in opt.param_groups[0]["params"]:
        p.grad.fill_(0.01)
    owner.step()
    assert all(not torch.equal(a, b) for a, b in zip(before, opt.param_groups[0]["params"]))
    assert all(opt.state[p]["momentum_buffer"] is not None for p in opt.param_groups[0]["params"])
    _, opt = _built(monkeypatch, OptimSpec.from_string("sgd", lr=0.05), replica)
    assert type(opt).__name__ == "ArenaSGD" and opt.param_groups[0]["lr"] == 0.05
    monkeypatch.setenv("GA_FUSED_OPTIM", "0")
    _, opt = _built(monkeypatch, spec, replica)
    inner = opt.opts[0] if replica else opt
    assert type(inner) is torch.optim.SGD


@pytest.mark.parametrize("call,msg", [
    (lambda L, a: L.ga_sgd_step(0, a(68), a(64), a(64), 1, 8, 8, -0.1, 0.9, 1.0, 0.0, 0, 0, None, None), "aligned"),
    (lambda L, a: L.ga_sgd_step(0, a(64), a(64), a(72), 1, 8, 8, -0.1, 0.9, 1.0, 0.0, 0, 0, None, None), "aligned"),
    (lambda L, a: L.ga_sgd_step(0, a(64), a(64), a(64), 2, 8, 12, -0.1, 0.9, 1.0, 0.0, 0, 0, None, None), "ld"),
    (lambda L, a: L.ga_sgd_step(0, a(64), a(64), a(64), 2, 10, 8, -0.1, 0.9, 1.0, 0.0, 0, 0, None, None), "ld"),
    (lambda L, a: L.ga_sgd_step(0, a(64), a(64), None, 1, 8, 8, -0.1, 0.9, 1.0, 0.0, 0, 0, None, None), "momentum"),
    (lambda L, a: L.ga_sgd_step(0, None, a(64), None, 1, 8, 8, -0.1, 0.0, 1.0, 0.0, 0, 0, None, None), "null"),
    (lambda L, a: L.ga_sgd_step(1, a(64), a(64), a(64), 1, 8, 8, -0.1, 0.9, 1.0, 0.0, 0, 0, None, None), "float32"),
    (lambda L, a: L.ga_sgd_step(0, a(64), a(64), a(64), 0, 8, 8, -0.1, 0.9, 1.0, 0.0, 0, 0, None, None), "sizes"),
], ids=["misaligned-param", "misaligned-buf", "ld-lt-n", "ld-not-x4", "null-buf-momentum", "null-param", "bf16", "K0"])
def test_ga_sgd_step_invalid_arguments_fail_cleanly(call, msg):
    """Checked on the host before any launch (no GPU needed): GA_EINVAL and a message."""
    from gym_amd import _lib
    L = _lib.lib()
    assert call(L, ctypes.c_void_p) == 1
    assert msg in L.ga_last_error().decode()


def test_ga_sgd_step_zero_length_is_a_noop():
    from gym_amd import _lib
    L = _lib.lib()
    assert L.ga_sgd_step(0, None, None, None, 1, 0, 0, -0.1, 0.9, 1.0, 0.0, 0, 0, None, None) == 0
    assert L.ga_last_error().decode() == ""


def test_one_minus_dampening_is_rounded_once():
    """Why the caller passes 1 - dampening: float(1 - d), torch's alpha, is not
    1.f - float(d) for these d."""
    import numpy as np
    for d in (0.6, 0.8, 0.9):
        assert np.float32(1 - d) != np.float32(1) - np.float32(d)
