"""Time DiLoCo's outer step with an Adam outer optimizer over GPT-2 124M rows at
K = 1, 8 and 32 replicas in one process (placement off): queued back-to-back
launches between two device events, the first two forms alternated for --pairs
pairs (the spread of the pairs is the noise):

  (a) fused: DiLoCoOuterAdam, one ga_diloco_outer_adam launch, (8K + 24) n bytes;
  (b) generic: the outer step both modes run for an outer optimizer without a
      fused kernel (engine.TorchOuter): the K-row sum, the divide, master - avg,
      torch.optim.Adam's step on an fp32 master, the copy of the master to all K
      rows;
  (c) ga_diloco_outer with momentum on the same rows, (8K + 16) n bytes: the same
      access pattern less one state stream.

One JSON line per K, appended to --out.  fused_outer=True is the strategies'
default only while (a) < (b) in every pair at every K.

    python tools/time_outer_adam.py [--reps 20] [--pairs 5] [--ks 1,8,32] [--out profiles/...txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_amd import ops  # noqa: E402
from gym_amd.arena import ArenaLayout  # noqa: E402
from gym_amd.comm import Collective  # noqa: E402
from gym_amd.engine import DiLoCoOuterAdam, TorchOuter  # noqa: E402
from gym_amd.shapes import MODELS  # noqa: E402
from gym_amd.strategy.optim import OptimSpec  # noqa: E402

PEAK = 8e12  # B/s, MI355X HBM3E
SGD = dict(lr=0.7, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=True)
LR = 0.05


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--model", default="gpt2-124m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outer_adam.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_outer_adam: no GPU (there is nothing to time on the CPU)")
    dev = torch.device("cuda:0")
    n = ArenaLayout(MODELS[a.model]()).n
    coll = Collective()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for K in [int(k) for k in a.ks.split(",")]:
        reps = torch.empty(K, n, device=dev)
        for k in range(K):
            reps[k].normal_(std=0.02)
        eng = DiLoCoOuterAdam(coll, K, n, dev, torch.float32, lr=LR, placement=False)
        eng.init_master(reps[0])
        # (b): the generic outer step, with its own master, optimizer and average buffer
        generic = TorchOuter(coll, K, n, dev, torch.float32, OptimSpec(torch.optim.Adam, lr=LR))
        generic.init_master(reps[0])
        # (c)
        sgd_master, sgd_mom = reps[0].clone(), torch.zeros(n, device=dev)

        def fused():
            eng(reps)

        def sgd():
            ops.diloco_outer(reps, sgd_master, sgd_mom, reps, n, K, SGD["lr"], SGD["momentum"], SGD["dampening"],
                             SGD["weight_decay"], SGD["nesterov"], False)

        pairs = [(timed(fused, a.reps), timed(lambda: generic(reps), a.reps)) for _ in range(a.pairs)]
        sgd_pairs = [(timed(fused, a.reps), timed(sgd, a.reps)) for _ in range(a.pairs)]
        ms_a = sum(x for x, _ in pairs) / len(pairs)
        ms_b = sum(y for _, y in pairs) / len(pairs)
        ms_a2 = sum(x for x, _ in sgd_pairs) / len(sgd_pairs)
        ms_c = sum(y for _, y in sgd_pairs) / len(sgd_pairs)
        bytes_a, bytes_c = (8 * K + 24) * n, (8 * K + 16) * n
        rate_a, rate_c = bytes_a / (ms_a2 * 1e-3), bytes_c / (ms_c * 1e-3)
        line = json.dumps({
            "what": "DiLoCo outer step, Adam outer optimizer", "model": a.model, "K": K, "n": n, "reps": a.reps,
            "placement": False, "fused_ms": round(ms_a, 4), "generic_ms": round(ms_b, 4),
            "pairs_ms_fused_generic": [[round(x, 4), round(y, 4)] for x, y in pairs],
            "fused_faster_in_every_pair": all(x < y for x, y in pairs),
            "generic_over_fused": round(ms_b / ms_a, 2),
            "generic_bytes_per_elem_at_fused_rate": round(ms_b / ms_a * (8 * K + 24), 1),
            "sgd_outer_ms": round(ms_c, 4),
            "pairs_ms_fused_sgd_outer": [[round(x, 4), round(y, 4)] for x, y in sgd_pairs],
            "fused_bytes": bytes_a, "fused_frac_of_8TBps": round(rate_a / PEAK, 4),
            "sgd_outer_bytes": bytes_c, "sgd_outer_frac_of_8TBps": round(rate_c / PEAK, 4),
            "fused_Bps_over_sgd_outer_Bps": round(rate_a / rate_c, 4),
        })
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del reps, eng, generic, sgd_master, sgd_mom
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
