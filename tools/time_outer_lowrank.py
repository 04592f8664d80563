"""Time DiLoCo's low-rank outer step over GPT-2 124M rows at K = 1 and 8 replicas in one
process, rank 4 and 32, with and without error feedback, placement off: queued back-to-back
launches between two device events, the forms taken in turn for --pairs rounds (the spread
of the rounds is the noise):

  (a) each of DiLoCoOuterLowRank's four launches (ga_lowrank_project, _orthonormalize,
      _backproject, ga_diloco_outer_lowrank) on the same rows; the outer launch writes the
      rows in place, so after the first repetition the deltas are what the residual holds
      (the launches have no data-dependent path);
  (b) ga_stream_copy moving each launch's algorithmic bytes: project and back-project read
      master and the K rows (and K residual rows with feedback), the orthonormalisation reads
      and writes the P factors once, the outer launch reads and writes master and momentum,
      writes the K rows and with feedback reads the rows and reads and writes the residual;
  (c) ga_diloco_outer (the uncompressed outer step) on the same rows.

The wire bytes per outer step (both all-reduce operands, flat in the world size) come from
the plan.  One JSON line per case, appended to --out.

    python tools/time_outer_lowrank.py [--reps 10] [--pairs 5] [--ks 1,8] [--ranks 4,32] [--out profiles/outer_lowrank.txt]
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
from gym_amd.engine import DiLoCoOuterLowRank  # noqa: E402
from gym_amd.shapes import MODELS  # noqa: E402
from time_outer_quant import SGD, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--ks", default="1,8")
    ap.add_argument("--ranks", default="4,32")
    ap.add_argument("--model", default="gpt2-124m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outer_lowrank.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_outer_lowrank: no GPU (there is nothing to time on the CPU)")
    dev = torch.device("cuda:0")
    layout = ArenaLayout(MODELS[a.model]())
    n, coll = layout.n, Collective()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    hp = (SGD["lr"], SGD["momentum"], SGD["dampening"], SGD["weight_decay"], SGD["nesterov"], False)
    for K in [int(k) for k in a.ks.split(",")]:
        reps = torch.empty(K, n, device=dev)
        for k in range(K):
            reps[k].normal_(std=0.02)
        plain_master, plain_mom = reps[0].clone(), torch.zeros(n, device=dev)
        for rank in [int(r) for r in a.ranks.split(",")]:
            for feedback in (False, True):
                e = DiLoCoOuterLowRank(coll, K, n, dev, torch.float32, layout=layout, rank=rank,
                                       error_feedback=feedback, **SGD)
                e.init_master(reps[0])
                p = e.plan
                read = 4 * n * (1 + K + (K if feedback else 0))
                nbytes = {"project": read, "orthonormalize": 8 * p.p_len, "backproject": read,
                          "outer": 4 * n * (4 + K + (3 * K if feedback else 0))}
                bufs = {w: [torch.empty((b // 2 + 15) // 16 * 16, dtype=torch.uint8, device=dev) for _ in range(2)]
                        for w, b in nbytes.items()}
                launches = {
                    "project": lambda: ops.lowrank_project(p, reps, e.master, e.residual, e.B, 1.0, e.A),
                    "orthonormalize": lambda: ops.lowrank_orthonormalize(p, e.A),
                    "backproject": lambda: ops.lowrank_backproject(p, reps, e.master, e.residual, e.A, e.B),
                    "outer": lambda: ops.diloco_outer_lowrank(p, e.A, e.B, float(K), reps, e.residual, e.master,
                                                              e.mom, K, *hp)}
                names = list(launches)
                forms = ([launches[w] for w in names] + [lambda w=w: ops.stream_copy(*bufs[w]) for w in names]
                         + [lambda: ops.diloco_outer(reps, plain_master, plain_mom, reps, n, K, *hp)])
                rounds = [[timed(f, a.reps) for f in forms] for _ in range(a.pairs)]
                ms = [sum(r[i] for r in rounds) / len(rounds) for i in range(len(forms))]
                total, copies = sum(ms[:4]), sum(ms[4:8])
                line = json.dumps({
                    "what": "DiLoCo outer step on low-rank (PowerSGD) pseudo-gradients", "model": a.model, "K": K,
                    "n": n, "rank": rank, "error_feedback": feedback, "reps": a.reps,
                    "compressed_tensors": len(p.compressed), "tensors": len(p.tensors),
                    "wire_bytes_per_step": p.wire_bytes, "fp32_arena_bytes": 4 * n,
                    **{f"{w}_ms": round(ms[i], 4) for i, w in enumerate(names)},
                    **{f"{w}_copy_ms": round(ms[4 + i], 4) for i, w in enumerate(names)},
                    **{f"{w}_bytes": nbytes[w] for w in names},
                    "lowrank_ms": round(total, 4), "copies_ms": round(copies, 4), "diloco_outer_ms": round(ms[8], 4),
                    "lowrank_over_copies": round(total / copies, 3),
                    "lowrank_over_diloco_outer": round(total / ms[8], 3),
                    "rounds_ms": [[round(x, 4) for x in r] for r in rounds],
                })
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
                del e, bufs
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
