"""Time ga_sgd_step (the fused SGD inner optimizer's kernel, momentum 0.9 with
Nesterov: 20 B per element) over GPT-2 124M rows at K = 1 and K = 32 replicas,
in the same process beside
  - ga_stream_copy of the same 20 B per element (10 read, 10 written),
  - ga_adam_step on the same rows (28 B per element),
  - what the step ran before the kernel existed: torch.optim.SGD built by
    OptimSpec.build on the arena-bound per-tensor parameters (K of them at K > 1,
    as ReplicaRunner's per-node optimizers).
Queued back-to-back launches between two device events; the kernels alternate
over several rounds, so the spread of the rounds is the noise.  Prints one JSON
line per K: milliseconds per launch, the bytes over that time as a fraction of
8 TB/s, and the ratios to the copy and to torch's SGD.

    timeout -k 10 600 python tools/time_inner_sgd.py [--reps 20] [--ks 1,32] [--rounds 3]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_amd import ops  # noqa: E402
from gym_amd.arena import ParamArena, ReplicaArena  # noqa: E402
from gym_amd.shapes import MODELS  # noqa: E402
from gym_amd.strategy import OptimSpec  # noqa: E402

PEAK = 8e12  # B/s, MI355X HBM3E
SGD_BYTES, ADAM_BYTES = 20, 28  # per element: p, g, buf read + p, buf written | p, g, m, v read + p, m, v written


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


class _Node(torch.nn.Module):
    def __init__(self, shapes, dev):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, device=dev) * 0.02) for s in shapes])


def time_copy(n_elems, reps, dev):
    """ga_stream_copy moving SGD_BYTES per element: half of them read, half written."""
    words = SGD_BYTES // 2 * n_elems // 4
    src = torch.empty(words, device=dev).normal_()
    dst = torch.empty_like(src)
    ms = timed(lambda: ops.stream_copy(src, dst), reps)
    del src, dst
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ks", default="1,32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", default="gpt2-124m")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_inner_sgd: no GPU (there is nothing to time on the CPU)")
    dev = torch.device("cuda:0")
    shapes = MODELS[a.model]()
    spec = OptimSpec(torch.optim.SGD, lr=1e-3, momentum=0.9, nesterov=True)
    for K in [int(k) for k in a.ks.split(",")]:
        models = [_Node(shapes, dev) for _ in range(K)]
        arena = ReplicaArena(models) if K > 1 else ParamArena(list(models[0].parameters()))
        P = arena.flat_set if K > 1 else arena.flat.view(1, -1)
        G = arena.grad_set if K > 1 else arena.grad_flat.view(1, -1)
        G.normal_(0.0, 1e-3)
        ld = P.shape[1]
        n_elems = K * ld
        copy_ms = [time_copy(n_elems, a.reps, dev)]
        B, V = torch.zeros_like(P), torch.zeros_like(P)
        sgd_hp = dict(neg_lr=-1e-3, momentum=0.9, one_m_dampening=1.0, weight_decay=0.0, nesterov=True)
        ops.sgd_step(P, G, B, first=True, **sgd_hp)  # the buffer holds a first gradient; timed: the steady step
        adam_hp = dict(lerp_w=0.1, beta2=0.999, one_m_beta2=1e-3, eps=1e-8, wd_factor=1 - 1e-5, l2_wd=0.0,
                       step_size=-1e-3, bc2_sqrt=1.0)

        def sgd():
            ops.sgd_step(P, G, B, first=False, **sgd_hp)

        def adam():
            ops.adam_step(P, G, B, V, **adam_hp)

        rounds = [(timed(sgd, a.reps), timed(adam, a.reps)) for _ in range(a.rounds)]
        del B, V
        torch.cuda.empty_cache()
        copy_ms.append(time_copy(n_elems, a.reps, dev))
        # torch's SGD on the arena-bound parameters, one optimizer per node (foreach: torch's default on the GPU)
        topts = [spec.build(m) for m in models]

        def torch_sgd():
            for o in topts:
                o.step()

        torch_ms = timed(torch_sgd, max(2, a.reps // 4), warmup=2)
        sgd_ms = sum(r[0] for r in rounds) / len(rounds)
        adam_ms = sum(r[1] for r in rounds) / len(rounds)
        cp = sum(copy_ms) / len(copy_ms)
        print(json.dumps({
            "kernel": "ga_sgd_step", "model": a.model, "K": K, "ld": ld, "tensors_per_node": len(shapes),
            "setting": "momentum 0.9, nesterov, first=0", "bytes": SGD_BYTES * n_elems,
            "ms": round(sgd_ms, 4), "frac_of_8TBps": round(SGD_BYTES * n_elems / (sgd_ms * 1e-3) / PEAK, 4),
            "stream_copy_ms": round(cp, 4), "stream_copy_ms_before_after": [round(c, 4) for c in copy_ms],
            "stream_copy_frac_of_8TBps": round(SGD_BYTES * n_elems / (cp * 1e-3) / PEAK, 4),
            "sgd_ms_over_copy_ms": round(sgd_ms / cp, 3),
            "adam_ms": round(adam_ms, 4), "adam_frac_of_8TBps": round(ADAM_BYTES * n_elems / (adam_ms * 1e-3) / PEAK, 4),
            "adam_ms_over_copy_of_its_bytes": round(adam_ms / (cp * ADAM_BYTES / SGD_BYTES), 3),
            "rounds_ms_sgd_adam": [[round(s, 4), round(m, 4)] for s, m in rounds],
            "torch_sgd_ms": round(torch_ms, 4), "torch_sgd_optimizers": K,
            "torch_sgd_ms_over_sgd_ms": round(torch_ms / sgd_ms, 2),
        }), flush=True)
        del topts, models, arena, P, G
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
