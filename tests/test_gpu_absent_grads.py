"""tests/test_absent_grads.py on the MI355X with the real kernels: the gated
model under SimpleReduce, DiLoCo, SPARTA (torch-drawn masks and
mask_source="philox", so both skip-table paths see a trainable parameter
without a gradient) and SPARTA+DiLoCo (default fused boundary), in process mode
(2 ranks on cuda:0 over gloo) and replica mode (K = 2), against the reference's
step restated with per-tensor torch on the same GPU (the torch-drawn masks are
the CUDA generator's bernoulli draws, per tensor with a gradient, in both; the
philox masks are the oracle's, with the absent tensors' ranges skipped)."""
import numpy as np
import pytest
import torch

import absent_scenarios as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def want():
    _need_gpu()
    return {name: A.restated(name, DEV) for name in A.NAMES}


@pytest.fixture(scope="module")
def proc(tmp_path_factory):
    _need_gpu()
    return A.run_process_mode(A.NAMES, DEV, False, str(tmp_path_factory.mktemp("absent_gpu")))


@pytest.fixture(scope="module")
def replica():
    _need_gpu()
    return {name: A.run_replica_mode(name, DEV) for name in A.NAMES}


def _untouched(params, name):
    init = dict(zip(A.names(), A.initial()))
    for node, ps in enumerate(params):
        for n, p in zip(A.names(), ps):
            if n in ("unused", "scale"):
                assert np.array_equal(p, init[n]), f"{name} node {node}: {n} moved by {np.abs(p - init[n]).max():.3g}"


def _check(name, got, want):
    params, steps = got
    A.compare(params, want[name][0])
    for s in steps:
        assert np.array_equal(s, A.expected_steps()), (name, s)
    _untouched(params, name)


@pytest.mark.parametrize("name", A.NAMES)
def test_process_mode_matches_the_reference_step_on_gpu(name, want, proc):
    _check(name, proc[name], want)


@pytest.mark.parametrize("name", A.NAMES)
def test_replica_mode_matches_the_reference_step_on_gpu(name, want, replica):
    _check(name, replica[name], want)


@pytest.mark.parametrize("name", ["sparta", "sparta_philox"])
def test_sparta_leaves_absent_layers_alone_on_their_steps_on_gpu(name):
    """Both skip-table sources on the real kernels, step by step: the gap layer
    bit-identical on every node over steps 2-3, the late layer at its initial
    value through steps 0-1 (absent_scenarios.check_layer_history)."""
    _need_gpu()
    A.check_layer_history(A.layer_history(name, DEV))
