"""Time DiLoCo's MX outer step over GPT-2 124M rows at K = 1 and 8 replicas in one
process, mxfp8 and mxfp4, with and without error feedback, placement off: queued
back-to-back launches between two device events, the forms taken in turn for --pairs
rounds (the spread of the rounds is the noise):

  (a) MX: DiLoCoOuterMX's two launches, ga_mx_encode over the K rows and
      ga_diloco_outer_mx (the new rows go to a second [K, n] set, so the deltas of the
      next repetition are not zero), and the encode alone; (20 + K (8 + 2 b)) n bytes
      with b = bits / 8 + 1 / 32, + 8 K n with feedback (the residual read and written);
  (b) the int8 / int4 pair of the same width on the same rows (tools/time_outer_quant.py's
      (a), b = bits / 8 + 1 / 64);
  (c) ga_stream_copy moving the bytes of (a), and of (b): what the box streams in the same
      process.

One JSON line per case, appended to --out.

    python tools/time_outer_mx.py [--reps 20] [--pairs 5] [--ks 1,8] [--out profiles/outer_mx.txt]
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
from gym_amd.engine import DiLoCoOuterMX, DiLoCoOuterQuant  # noqa: E402
from gym_amd.shapes import MODELS  # noqa: E402
from time_outer_quant import PEAK, SGD, timed  # noqa: E402


def pair_bytes(K, n, b, feedback):
    return int((20 + K * (8 + 2 * b) + (8 * K if feedback else 0)) * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--ks", default="1,8")
    ap.add_argument("--model", default="gpt2-124m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outer_mx.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_outer_mx: no GPU (there is nothing to time on the CPU)")
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
                mx = DiLoCoOuterMX(coll, K, n, dev, torch.float32, bits=bits, error_feedback=feedback, **SGD)
                it = DiLoCoOuterQuant(coll, K, n, dev, torch.float32, bits=bits, error_feedback=feedback, **SGD)
                for eng in (mx, it):
                    eng.init_master(reps[0])
                by_mx, by_int = pair_bytes(K, n, bits / 8 + 1 / 32, feedback), pair_bytes(K, n, bits / 8 + 1 / 64,
                                                                                        feedback)
                half = [(b // 2 + 15) // 16 * 16 for b in (by_mx, by_int)]
                src, dst = (torch.empty(max(half), dtype=torch.uint8, device=dev) for _ in range(2))

                def mx_encode():
                    ops.mx_encode(reps, mx.master, mx.residual, mx.payload, n, bits)

                def mx_pair():  # the engine's two launches, the new rows to a second set
                    mx_encode()
                    ops.diloco_outer_mx(mx.payload, mx.master, mx.mom, out, n, bits, K, *hp)

                def int_pair():
                    ops.quant_encode(reps, it.master, it.residual, it.payload, n, bits)
                    ops.diloco_outer_dequant(it.payload, it.master, it.mom, out, n, bits, K, *hp)

                forms = [mx_pair, mx_encode, lambda: ops.stream_copy(src[:half[0]], dst[:half[0]]), int_pair,
                         lambda: ops.stream_copy(src[:half[1]], dst[:half[1]])]
                rounds = [[timed(f, a.reps) for f in forms] for _ in range(a.pairs)]
                ms_mx, ms_enc, ms_copy, ms_int, ms_icopy = (sum(r[i] for r in rounds) / len(rounds) for i in range(5))
                line = json.dumps({
                    "what": "DiLoCo outer step on MX block-float pseudo-gradients", "model": a.model, "K": K, "n": n,
                    "format": f"mxfp{bits}", "error_feedback": feedback, "reps": a.reps,
                    "payload_bytes_per_node": mx.payload_bytes_per_node,
                    "mx_ms": round(ms_mx, 4), "mx_encode_ms": round(ms_enc, 4), "mx_decode_ms": round(ms_mx - ms_enc, 4),
                    "copy_ms": round(ms_copy, 4), "int_ms": round(ms_int, 4), "int_copy_ms": round(ms_icopy, 4),
                    "rounds_ms_mx_encode_copy_int_intcopy": [[round(x, 4) for x in r] for r in rounds],
                    "mx_bytes": by_mx, "mx_frac_of_8TBps": round(by_mx / (ms_mx * 1e-3) / PEAK, 4),
                    "int_bytes": by_int, "mx_over_copy": round(ms_mx / ms_copy, 3),
                    "int_over_copy": round(ms_int / ms_icopy, 3), "mx_over_int": round(ms_mx / ms_int, 3),
                })
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
                del mx, it, src, dst
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
