"""Time the SPARTA step of the two cycle selectors over GPT-2 124M rows at K = 8 and
K = 32 replicas in one process, p = 0.005: the listed path (listed=True: ListedPlan +
ga_sparta_average_listed) against the mask path (listed=False: per-tensor get_indices,
pack, count read back, the mask-mode kernel).

Each side is the WHOLE per-step path of SparseAverage.__call__ (the draw or the plan,
the table upload, the launches, the mask path's host sync), timed with the host clock
around --reps steps that end in a device synchronise; the two sides are alternated for
--pairs pairs (the spread of the pairs is the noise).  The once-per-cycle draw (first
call) is reported on its own.  Beside each result: the listed kernel alone (device
events, one step's table replayed) and ga_probe_random_words on the same index set
(read + write of every listed word of every replica: the random-word floor).

One JSON line per (selector, K), appended to --out.

    python tools/time_sparta_listed.py [--reps 20] [--pairs 5] [--ks 8,32] [--out profiles/sparta_listed.txt]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_amd import ops  # noqa: E402
from gym_amd.arena import ArenaLayout  # noqa: E402
from gym_amd.comm import Collective  # noqa: E402
from gym_amd.shapes import MODELS  # noqa: E402
from gym_amd.strategy import sparta  # noqa: E402


def host_timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def event_timed(fn, reps, warmup=3):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparta_listed.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_sparta_listed: no GPU (there is nothing to time on the CPU)")
    dev = torch.device("cuda:0")
    L = ArenaLayout(MODELS[a.model]())
    n = L.n
    params = [torch.zeros(s, device=dev, requires_grad=True) for s in L.shapes]
    for q in params:
        q.grad = torch.zeros_like(q)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for K in [int(k) for k in a.ks.split(",")]:
        reps = torch.empty(K, n, device=dev)
        for k in range(K):
            reps[k].normal_(std=0.02)
        for name in ("ShuffledSequentialIndexSelector", "PartitionedIndexSelector"):
            cls = getattr(sparta, name)
            sides, first = {}, {}
            for listed in (True, False):
                sp = sparta.SparseAverage()
                sp.bind(cls(a.p, listed=listed), Collective(), K, L, n, dev, torch.float32)

                def step(sp=sp):
                    with torch.no_grad():
                        sp(reps, params)
                    sp.iteration += 1
                first[listed] = host_timed(step, 1)  # the cycle's draw (randperm / rand.argsort per tensor)
                host_timed(step, 3)
                sides[listed] = (sp, step)
            assert sides[True][0].mask_draw == "listed" and sides[False][0].mask_draw == "torch"
            pairs = [(host_timed(sides[True][1], a.reps), host_timed(sides[False][1], a.reps)) for _ in range(a.pairs)]
            # the listed kernel alone and the random-word probe, on one step's index set
            plan = sides[True][0].plan
            rows, total, _ = plan.step(params, set(), sides[True][0].iteration)
            table = plan.table(rows).clone()
            pos = torch.cat([plan.order[s:s + c] for s, c in rows])
            kern = event_timed(lambda: ops.sparta_average_listed(reps, plan.order, table, total, float(K), n=n), a.reps)
            probe = event_timed(lambda: ops.probe_random_words(reps, pos, total, write=True), a.reps)
            line = json.dumps({
                "what": "SPARTA cycle-selector step, listed vs mask path", "selector": name, "model": a.model, "K": K,
                "n": n, "p": a.p, "reps": a.reps, "selected": total, "tensors": len(rows),
                "listed_step_ms": round(sum(x for x, _ in pairs) / len(pairs), 4),
                "mask_step_ms": round(sum(y for _, y in pairs) / len(pairs), 4),
                "pairs_ms_listed_mask": [[round(x, 4), round(y, 4)] for x, y in pairs],
                "listed_faster_in_every_pair": all(x < y for x, y in pairs),
                "first_call_ms_listed_mask": [round(first[True], 3), round(first[False], 3)],
                "listed_kernel_ms": round(kern, 4), "probe_random_words_ms": round(probe, 4),
                "kernel_over_probe": round(kern / probe, 3),
                "listed_bytes": 4 * total + 2 * K * 4 * total,
            })
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del reps


if __name__ == "__main__":
    main()
