"""Time the streaming outer step's launches over GPT-2 124M rows at K = 8 replicas in one
process, placement off: queued back-to-back launches between two device events, the
forms of a case taken in turn for --pairs rounds (the spread of the rounds is the noise).

  fragment   ga_diloco_outer in place over the whole arena against one fragment of
             F = 4 (engine.fragment_bounds over the model's tensors): the time of one
             outer event, i.e. the peak a step sees.
  merge_a0   ga_diloco_outer_merge at alpha = 0 in place over the K rows, (8 K + 16) n
             bytes, against ga_diloco_outer on the same rows (the same bytes) and
             ga_stream_copy of as many bytes.
  merge_mix  ga_diloco_outer_merge at alpha = 0.5 from one staged row into the K live
             rows (K = 1, K_out = 8), (4 + 16 + 8 K) n bytes, against ga_diloco_outer in
             place on the same rows, (8 K + 16) n bytes, and ga_stream_copy of the
             merge's bytes.

The yardstick is the bytes per second ga_diloco_outer reaches in the same process on the
same rows: *_rate_over_outer is the merge's bytes/s over it.  The overlap of the
exchange with compute is not timed: it needs more than one GPU.  One JSON line per
case, appended to --out.

    python tools/time_outer_stream.py [--reps 30] [--pairs 5] [--k 8] [--out profiles/...txt]
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
from gym_amd.engine import fragment_bounds  # noqa: E402
from gym_amd.shapes import MODELS  # noqa: E402

PEAK = 8e12  # B/s, MI355X HBM3E
SGD = dict(lr=0.7, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=True)


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


def rounds_of(fns, reps, pairs):
    """[[ms of every fn] per round]: the fns taken in turn, `pairs` rounds."""
    return [[timed(fn, reps) for fn in fns] for _ in range(pairs)]


def mean_col(rounds, i):
    return sum(r[i] for r in rounds) / len(rounds)


def rate(nbytes, ms):
    return nbytes / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--fragments", type=int, default=4)
    ap.add_argument("--model", default="gpt2-124m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outer_stream.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_outer_stream: no GPU (there is nothing to time on the CPU)")
    if a.pairs < 5:
        sys.exit("time_outer_stream: at least 5 alternated rounds")
    dev = torch.device("cuda:0")
    layout = ArenaLayout(MODELS[a.model]())
    n, K, F = layout.n, a.k, a.fragments
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    reps = torch.empty(K, n, device=dev)
    for k in range(K):
        reps[k].normal_(std=0.02)
    master, mom = reps[0].clone(), torch.zeros(n, device=dev)
    stage = reps.sum(dim=0)
    args = (SGD["lr"], SGD["momentum"], SGD["dampening"], SGD["weight_decay"], SGD["nesterov"], False)

    def outer(lo=0, hi=n):
        ops.diloco_outer(reps[:, lo:hi], master[lo:hi], mom[lo:hi], reps[:, lo:hi], hi - lo, K, *args)

    def merge_a0():
        ops.diloco_outer_merge(reps, master, mom, reps, n, K, *args, 0.0)

    def merge_mix():
        ops.diloco_outer_merge(stage, master, mom, reps, n, K, *args, 0.5)

    def emit(rec):
        line = json.dumps(dict({"model": a.model, "K": K, "n": n, "reps": a.reps, "pairs": a.pairs}, **rec))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    # -- one outer event: the whole arena against one fragment of F
    bounds = fragment_bounds(layout.offsets, n, F, 512)
    f_lo, f_hi = max(zip(bounds, bounds[1:]), key=lambda ab: ab[1] - ab[0])  # the largest fragment: the peak
    rounds = rounds_of([outer, lambda: outer(f_lo, f_hi)], a.reps, a.pairs)
    ms_whole, ms_frag = mean_col(rounds, 0), mean_col(rounds, 1)
    b_whole, b_frag = (8 * K + 16) * n, (8 * K + 16) * (f_hi - f_lo)
    emit({"what": "fragment: ga_diloco_outer over the whole arena vs the largest fragment", "F": F, "bounds": bounds,
          "fragment": [f_lo, f_hi], "whole_ms": round(ms_whole, 4), "fragment_ms": round(ms_frag, 4),
          "whole_over_fragment": round(ms_whole / ms_frag, 3), "elems_whole_over_fragment": round(n / (f_hi - f_lo), 3),
          "whole_frac_of_8TBps": round(rate(b_whole, ms_whole) / PEAK, 4),
          "fragment_frac_of_8TBps": round(rate(b_frag, ms_frag) / PEAK, 4),
          "rounds_ms_whole_fragment": [[round(x, 4) for x in r] for r in rounds]})

    # -- the merge kernel against ga_diloco_outer and a copy of its bytes
    for name, fn, nbytes in (("merge_a0", merge_a0, (8 * K + 16) * n), ("merge_mix", merge_mix, (4 + 16 + 8 * K) * n)):
        half = (nbytes // 2 + 15) // 16 * 16
        src = torch.empty(half, dtype=torch.uint8, device=dev)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)
        rounds = rounds_of([fn, outer, lambda: ops.stream_copy(src, dst)], a.reps, a.pairs)
        ms_m, ms_o, ms_c = (mean_col(rounds, i) for i in range(3))
        r_m, r_o, r_c = rate(nbytes, ms_m), rate(b_whole, ms_o), rate(2 * half, ms_c)
        emit({"what": f"{name}: ga_diloco_outer_merge vs ga_diloco_outer on the same rows vs ga_stream_copy",
              "alpha": 0.0 if name == "merge_a0" else 0.5, "K_src": K if name == "merge_a0" else 1, "K_out": K,
              "merge_ms": round(ms_m, 4), "outer_ms": round(ms_o, 4), "copy_ms": round(ms_c, 4),
              "merge_bytes": nbytes, "outer_bytes": b_whole, "copy_bytes": 2 * half,
              "merge_TBps": round(r_m / 1e12, 3), "outer_TBps": round(r_o / 1e12, 3), "copy_TBps": round(r_c / 1e12, 3),
              "merge_frac_of_8TBps": round(r_m / PEAK, 4),
              "merge_rate_over_outer": round(r_m / r_o, 3), "merge_rate_over_copy": round(r_m / r_c, 3),
              "outer_rate_over_copy": round(r_o / r_c, 3),
              "rounds_ms_merge_outer_copy": [[round(x, 4) for x in r] for r in rounds]})
        del src, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
