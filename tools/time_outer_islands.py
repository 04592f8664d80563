"""Time the island outer step over GPT-2 124M rows, all nodes in one process, placement
off, fp32, momentum 0.9 with Nesterov: queued back-to-back launches between two device
events, the forms of a case taken in turn for --pairs rounds (the spread of the rounds is
the noise).  Cases: K = 8 nodes in islands of s = 2, K = 32 in islands of s = 4 (one fixed
shuffle).  Per case, in turn:

  islands    ONE ga_diloco_outer_islands launch in place over the K rows, every member
             local: 24 K n bytes (each row read and written, each node's master and
             momentum read and written).
  composite  the same round from the kernels that existed before: per island a scratch
             copy of its s rows (in place the first member's write-back would change
             what its partners read), then per member ga_diloco_outer over the scratch
             on that member's master and momentum, written to its row:
             K + K / s launches, about (4 s + 28) K n bytes.
  copy       ga_stream_copy of the fused launch's 24 K n bytes (half read, half written).
  outer      ga_diloco_outer in place over the same K rows with ONE master and momentum,
             (8 K + 16) n bytes: the sibling's rate in the same process.
  outer_copy ga_stream_copy of the sibling's bytes.

islands_rate_over_copy beside outer_rate_over_copy is the comparison DESIGN quotes; the
spread is (max - min) / mean of a column's rounds.  The wire saving across GPUs is not
timed: it needs more than one GPU.  One JSON line per case, appended to --out.

    python tools/time_outer_islands.py [--reps 10] [--pairs 5] [--out profiles/...txt]
"""
import argparse
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_amd import ops  # noqa: E402
from gym_amd.arena import ArenaLayout  # noqa: E402
from gym_amd.shapes import MODELS  # noqa: E402

PEAK = 8e12  # B/s, MI355X HBM3E
SGD = dict(lr=0.7, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=True)
COPY_PIECE = 4 << 30  # bytes per ga_stream_copy launch (src and dst each)


def timed(fn, reps, warmup=2):
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


def col(rounds, i):
    return [r[i] for r in rounds]


def mean(xs):
    return sum(xs) / len(xs)


def spread(xs):
    return (max(xs) - min(xs)) / mean(xs)


def copier(nbytes, dev):
    """(fn, bytes moved): ga_stream_copy launches that read nbytes / 2 and write nbytes / 2,
    in pieces of at most COPY_PIECE, each piece its own pair of buffers."""
    half = (nbytes // 2 + 15) // 16 * 16
    sizes = [min(COPY_PIECE, half - o) for o in range(0, half, COPY_PIECE)]
    bufs = [(torch.empty(s, dtype=torch.uint8, device=dev), torch.empty(s, dtype=torch.uint8, device=dev))
            for s in sizes]

    def fn():
        for src, dst in bufs:
            ops.stream_copy(src, dst)

    return fn, 2 * half


def case(K, s, n, dev, a, emit):
    reps = torch.empty(K, n, device=dev)
    for k in range(K):
        reps[k].normal_(std=0.02)
    master = reps.clone()
    mom = torch.zeros(K, n, device=dev)
    ranks = list(range(K))
    random.Random(0).shuffle(ranks)
    islands = [sorted(ranks[i:i + s]) for i in range(0, K, s)]
    index = [torch.tensor(isl, device=dev) for isl in islands]
    scratch = torch.empty(s, n, device=dev)
    args = (SGD["lr"], SGD["momentum"], SGD["dampening"], SGD["weight_decay"], SGD["nesterov"], False)

    def fused():
        ops.diloco_outer_islands(reps, islands, islands, master, mom, reps, n, *args)

    def composite():
        for isl, idx in zip(islands, index):
            torch.index_select(reps, 0, idx, out=scratch[:len(isl)])
            for m in isl:
                ops.diloco_outer(scratch[:len(isl)], master[m], mom[m], reps[m], n, len(isl), *args)

    def outer():
        ops.diloco_outer(reps, master[0], mom[0], reps, n, K, *args)

    b_fused, b_comp, b_outer = 24 * K * n, (4 * s + 28) * K * n, (8 * K + 16) * n
    copy, b_copy = copier(b_fused, dev)
    ocopy, b_ocopy = copier(b_outer, dev)
    rounds = rounds_of([fused, composite, copy, outer, ocopy], a.reps, a.pairs)
    ms = [mean(col(rounds, i)) for i in range(5)]
    r_f, r_c, r_o, r_oc = b_fused / ms[0] * 1e3, b_copy / ms[2] * 1e3, b_outer / ms[3] * 1e3, b_ocopy / ms[4] * 1e3
    emit({"what": "ga_diloco_outer_islands vs the composite of ga_diloco_outer launches vs ga_stream_copy; "
                  "ga_diloco_outer on the same rows vs its own copy",
          "K": K, "island_size": s, "islands": islands, "n": n,
          "islands_ms": round(ms[0], 4), "composite_ms": round(ms[1], 4), "copy_ms": round(ms[2], 4),
          "outer_ms": round(ms[3], 4), "outer_copy_ms": round(ms[4], 4),
          "islands_bytes": b_fused, "composite_bytes": b_comp, "copy_bytes": b_copy, "outer_bytes": b_outer,
          "outer_copy_bytes": b_ocopy, "islands_launches": 1, "composite_launches": K + len(islands),
          "islands_TBps": round(r_f / 1e12, 3), "copy_TBps": round(r_c / 1e12, 3), "outer_TBps": round(r_o / 1e12, 3),
          "outer_copy_TBps": round(r_oc / 1e12, 3), "islands_frac_of_8TBps": round(r_f / PEAK, 4),
          "composite_over_islands_ms": round(ms[1] / ms[0], 3),
          "islands_beat_composite_in_every_round": all(r[0] < r[1] for r in rounds),
          "islands_rate_over_copy": round(r_f / r_c, 3), "outer_rate_over_copy": round(r_o / r_oc, 3),
          "spread": {name: round(spread(col(rounds, i)), 4)
                     for i, name in enumerate(("islands", "composite", "copy", "outer", "outer_copy"))},
          "rounds_ms_islands_composite_copy_outer_outercopy": [[round(x, 4) for x in r] for r in rounds]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--cases", default="8:2,32:4", help="K:island_size, comma separated")
    ap.add_argument("--model", default="gpt2-124m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outer_islands.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_outer_islands: no GPU (there is nothing to time on the CPU)")
    if a.pairs < 5:
        sys.exit("time_outer_islands: at least 5 alternated rounds")
    dev = torch.device("cuda:0")
    n = ArenaLayout(MODELS[a.model]()).n
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(rec):
        line = json.dumps(dict({"model": a.model, "dtype": "fp32", "reps": a.reps, "pairs": a.pairs}, **rec))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    for spec in a.cases.split(","):
        K, s = (int(v) for v in spec.split(":"))
        case(K, s, n, dev, a, emit)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
