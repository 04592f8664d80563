"""Time DiLoCo's rotated integer outer step over GPT-2 124M rows at K = 1 and 8 replicas in
one process, rht-int8 and rht-int4, with and without error feedback, placement off: queued
back-to-back launches between two device events, the forms taken in turn for --pairs
rounds (the spread of the rounds is the noise):

  (a) rotated: DiLoCoOuterRHT's two launches, ga_rht_encode over the K rows and
      ga_diloco_outer_rht (the new rows go to a second [K, n] set, so the deltas of the
      next repetition are not zero), and the encode alone; (20 + K (8 + 2 b)) n bytes
      with b = bits / 8 + 1 / 64, + 8 K n with feedback (the residual read and written);
  (b) the int8 / int4 pair of the same width on the same rows and its encode alone
      (tools/time_outer_quant.py's (a)): the same bytes;
  (c) ga_stream_copy moving those bytes: what the box streams in the same process.

One JSON line per case, appended to --out.

    python tools/time_outer_rht.py [--reps 20] [--pairs 5] [--ks 1,8] [--out profiles/outer_rht.txt]
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
from gym_amd.engine import DiLoCoOuterQuant, DiLoCoOuterRHT  # noqa: E402
from gym_amd.shapes import MODELS  # noqa: E402
from time_outer_quant import PEAK, SGD, timed  # noqa: E402


def pair_bytes(K, n, b, feedback):
    return int((20 + K * (8 + 2 * b) + (8 * K if feedback else 0)) * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--ks", default="1,8")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--model", default="gpt2-124m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outer_rht.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_outer_rht: no GPU (there is nothing to time on the CPU)")
    dev = torch.device("cuda:0")
    n = ArenaLayout(MODELS[a.model]()).n
    coll = Collective()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    hp = (SGD["lr"], SGD["momentum"], SGD["dampening"], SGD["weight_decay"], SGD["nesterov"], False)
    for K in [int(k) for k in a.ks.split(",")]:
        reps = torch.empty(K, n, device=dev)
        for k in range(K):
            reps[k].normal_(std=0.02)
        out = torch.empty_like(reps)
        for bits in (8, 4):
            for feedback in (False, True):
                rh = DiLoCoOuterRHT(coll, K, n, dev, torch.float32, bits=bits, error_feedback=feedback, seed=a.seed,
                                    **SGD)
                it = DiLoCoOuterQuant(coll, K, n, dev, torch.float32, bits=bits, error_feedback=feedback, **SGD)
                for eng in (rh, it):
                    eng.init_master(reps[0])
                nbytes = pair_bytes(K, n, bits / 8 + 1 / 64, feedback)
                half = (nbytes // 2 + 15) // 16 * 16
                src, dst = (torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(2))

                def rht_encode():
                    ops.rht_encode(reps, rh.master, rh.residual, rh.payload, n, bits, a.seed)

                def rht_pair():  # the engine's two launches, the new rows to a second set
                    rht_encode()
                    ops.diloco_outer_rht(rh.payload, rh.master, rh.mom, out, n, bits, K, *hp, a.seed)

                def int_encode():
                    ops.quant_encode(reps, it.master, it.residual, it.payload, n, bits)

                def int_pair():
                    int_encode()
                    ops.diloco_outer_dequant(it.payload, it.master, it.mom, out, n, bits, K, *hp)

                forms = [rht_pair, rht_encode, int_pair, int_encode, lambda: ops.stream_copy(src, dst)]
                rounds = [[timed(f, a.reps) for f in forms] for _ in range(a.pairs)]
                ms_r, ms_re, ms_i, ms_ie, ms_c = (sum(r[i] for r in rounds) / len(rounds) for i in range(5))
                line = json.dumps({
                    "what": "DiLoCo outer step on Hadamard-rotated int8 / int4 pseudo-gradients", "model": a.model,
                    "K": K, "n": n, "format": f"rht-int{bits}", "error_feedback": feedback, "reps": a.reps,
                    "payload_bytes_per_node": rh.payload_bytes_per_node,
                    "rht_ms": round(ms_r, 4), "rht_encode_ms": round(ms_re, 4), "rht_decode_ms": round(ms_r - ms_re, 4),
                    "int_ms": round(ms_i, 4), "int_encode_ms": round(ms_ie, 4), "int_decode_ms": round(ms_i - ms_ie, 4),
                    "copy_ms": round(ms_c, 4),
                    "rounds_ms_rht_rhtencode_int_intencode_copy": [[round(x, 4) for x in r] for r in rounds],
                    "bytes": nbytes, "rht_frac_of_8TBps": round(nbytes / (ms_r * 1e-3) / PEAK, 4),
                    "rht_over_copy": round(ms_r / ms_c, 3), "int_over_copy": round(ms_i / ms_c, 3),
                    "rht_over_int": round(ms_r / ms_i, 3),
                    "rht_decode_over_int_decode": round((ms_r - ms_re) / (ms_i - ms_ie), 3),
                })
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
                del rh, it, src, dst
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
