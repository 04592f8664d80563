"""Time the SPARTA+DiLoCo boundary step (both modules fire) over GPT-2 124M rows
at K = 8 and K = 32 replicas in one process, p = 0.005, a fresh mask per launch:
queued back-to-back launches between two device events, the two forms alternated
for --pairs pairs (the spread of the pairs is the noise):

  (a) two launches: ga_sparta_average_local (the reference draw in-kernel, as on
      ordinary steps) then ga_diloco_outer;
  (b) one pass: ga_sparta_torch_bernoulli into packed words, then
      ga_diloco_outer_masked;

and ga_diloco_outer alone as the floor.  One JSON line per K, appended to --out.
fuse_boundary=True is the strategy's default only while (b) < (a) in every pair
at both K.

    python tools/time_sparta_diloco.py [--reps 20] [--pairs 5] [--ks 8,32] [--out profiles/...txt]
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
from gym_amd.shapes import MODELS  # noqa: E402
from gym_amd.strategy.sparta import MaskDraw  # noqa: E402

PEAK = 8e12  # B/s, MI355X HBM3E
HP = dict(lr=0.7, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=True)


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
    ap.add_argument("--ks", default="8,32")
    ap.add_argument("--p", type=float, default=0.005)
    ap.add_argument("--model", default="gpt2-124m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparta_diloco_boundary.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_sparta_diloco: no GPU (there is nothing to time on the CPU)")
    dev = torch.device("cuda:0")
    L = ArenaLayout(MODELS[a.model]())
    n = L.n
    table, nblocks = ops.sparta_bernoulli_table(L.offsets, L.numels, dev)
    step = MaskDraw.offset_step * len(L.numels)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for K in [int(k) for k in a.ks.split(",")]:
        reps = torch.empty(K, n, device=dev)
        for k in range(K):
            reps[k].normal_(std=0.02)
        master = reps[0].clone()
        mom = torch.zeros(n, device=dev)
        bits = torch.zeros(ops.sparta_mask_words(n), dtype=torch.int64, device=dev)
        draws = [0]

        def offset():  # a fresh mask per launch: the generator offset a training step would be at
            draws[0] += 1
            return draws[0] * step

        def outer():
            ops.diloco_outer(reps, master, mom, reps, n, K, HP["lr"], HP["momentum"], HP["dampening"],
                             HP["weight_decay"], HP["nesterov"], False)

        def two_launches():
            draw = ops.TorchDraw(table, a.p, 42, offset(), MaskDraw.offset_step)
            ops.sparta_average_local(reps, n, float(K), mask=draw)
            outer()

        def one_pass():
            ops.sparta_torch_bernoulli(table, nblocks, a.p, 42, offset(), MaskDraw.offset_step, bits)
            ops.diloco_outer_masked(reps, bits, master, mom, n, float(K), K, HP["lr"], HP["momentum"],
                                    HP["dampening"], HP["weight_decay"], HP["nesterov"], False)

        def draw_only():
            ops.sparta_torch_bernoulli(table, nblocks, a.p, 42, offset(), MaskDraw.offset_step, bits)

        pairs = [(timed(two_launches, a.reps), timed(one_pass, a.reps)) for _ in range(a.pairs)]
        floor = timed(outer, a.reps)
        draw_ms = timed(draw_only, a.reps)
        ms_a = sum(x for x, _ in pairs) / len(pairs)
        ms_b = sum(y for _, y in pairs) / len(pairs)
        nbytes = (2 * K + 4) * 4 * n
        line = json.dumps({
            "what": "SPARTA+DiLoCo boundary step", "model": a.model, "K": K, "n": n, "p": a.p, "reps": a.reps,
            "two_launches_ms": round(ms_a, 4), "one_pass_ms": round(ms_b, 4),
            "pairs_ms_two_launches_one_pass": [[round(x, 4), round(y, 4)] for x, y in pairs],
            "one_pass_faster_in_every_pair": all(y < x for x, y in pairs),
            "outer_alone_ms": round(floor, 4), "packed_draw_ms": round(draw_ms, 4),
            "one_pass_over_outer_alone": round(ms_b / floor, 3),
            "masked_kernel_over_outer_alone": round((ms_b - draw_ms) / floor, 3),
            "outer_alone_frac_of_8TBps": round(nbytes / (floor * 1e-3) / PEAK, 4),
            "one_pass_bytes": nbytes + n // 8,
        })
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del reps, master, mom


if __name__ == "__main__":
    main()
