"""Parameters that get no gradient on some steps, through the trainers, on CPU
with the stand-in kernels: tiny_models.GatedMLP for 6 steps on 2 nodes under
SimpleReduce (AdamW, max_norm 1), DiLoCo (H = 2), SPARTA and SPARTA+DiLoCo, in
process mode over gloo and in replica mode (loop and vmap forward), against the
reference's step restated with per-tensor torch (absent_scenarios.restated),
where such a parameter's .grad is None: no all-reduce, no decay, no moment
update, its AdamW step does not advance, SPARTA does not average it."""
import numpy as np
import pytest

import absent_scenarios as A


@pytest.fixture(scope="module")
def want():
    return {name: A.restated(name) for name in A.NAMES}


@pytest.fixture(scope="module")
def proc(tmp_path_factory):
    return A.run_process_mode(A.NAMES, "cpu", True, str(tmp_path_factory.mktemp("absent")))


@pytest.fixture
def fake():
    import fake_sparta_diloco_ops
    fake_sparta_diloco_ops.install()


def _untouched(params, name):
    """The never-used and the frozen parameter equal their initial values bit for bit."""
    init = dict(zip(A.names(), A.initial()))
    for node, ps in enumerate(params):
        for n, p in zip(A.names(), ps):
            if n in ("unused", "scale"):
                assert np.array_equal(p, init[n]), f"{name} node {node}: {n} moved by {np.abs(p - init[n]).max():.3g}"


def test_restated_steps_follow_the_gates(want):
    """The restatement itself: AdamW's per-parameter step counts are the number
    of steps the model's gates let each parameter through (never-used and frozen
    0, late 4, gap 4, the rest 6)."""
    for name in A.NAMES:
        for steps in want[name][1]:
            assert np.array_equal(steps, A.expected_steps()), (name, steps)


@pytest.mark.parametrize("name", ["simple", "diloco"])
def test_restatement_matches_the_reference_recording(name, want):
    """tests/golden/absent_grads.npz (gen_golden.py g6): the reference's own
    SimpleReduce and DiLoCo on the gated model, 2 nodes over gloo on the CPU:
    every node's parameters and per-parameter AdamW steps."""
    import os
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "absent_grads.npz")) as z:
        rec = [[z[f"{name}_node{r}_{i}"] for i in range(len(A.names()))] for r in range(A.NODES)]
        steps = [z[f"{name}_steps_{r}"] for r in range(A.NODES)]
    A.compare(want[name][0], rec)
    for mine, theirs in zip(want[name][1], steps):
        assert np.array_equal(mine, theirs), (name, mine, theirs)


@pytest.mark.parametrize("name", A.NAMES)
def test_process_mode_matches_the_reference_step(name, want, proc):
    params, steps = proc[name]
    A.compare(params, want[name][0])
    for s in steps:
        assert np.array_equal(s, A.expected_steps()), (name, s)
    if name == "simple":
        _untouched(params, name)


@pytest.mark.parametrize("forward", ["loop", "vmap"])
@pytest.mark.parametrize("name", A.NAMES)
def test_replica_mode_matches_the_reference_step(fake, name, forward, want):
    params, steps = A.run_replica_mode(name, "cpu", forward)
    A.compare(params, want[name][0])
    for s in steps:
        assert np.array_equal(s, A.expected_steps()), (name, forward, s)
    if name == "simple":
        _untouched(params, name)


@pytest.mark.parametrize("name", A.NAMES)
def test_vmap_forward_equals_loop_forward(fake, name):
    loop, _ = A.run_replica_mode(name, "cpu", "loop")
    vm, _ = A.run_replica_mode(name, "cpu", "vmap")
    A.compare(vm, loop)


@pytest.mark.parametrize("name", ["sparta", "sparta_philox"])
def test_sparta_leaves_absent_layers_alone_on_their_steps(fake, name):
    """gym_amd's own run, step by step: the gap layer, which differs between the
    nodes by then, is bit-identical on every node over its absent steps 2-3
    (neither stepped nor averaged) and moves again at step 4; the late layer
    keeps its initial value through steps 0-1."""
    seen = A.layer_history(name, "cpu")
    A.check_layer_history(seen)
