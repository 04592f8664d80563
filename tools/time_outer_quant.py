"""Time DiLoCo's quantised outer step over GPT-2 124M rows at K = 1 and 8 replicas in
one process, int8 and int4: queued back-to-back launches between two device events,
three forms taken in turn for --pairs rounds (the spread of the rounds is the noise):

  (a) quantised: DiLoCoOuterQuant's two launches, ga_quant_encode over the K rows and
      ga_diloco_outer_dequant (the new rows go to a second [K, n] set, so the deltas
      of the next repetition are not zero); (20 + K (8 + 2 b)) n bytes with b = bits / 8 +
      1 / 64 (encode: master 4, K rows 4 K, K payload rows written K b; decode: K
      payload rows K b, master and momentum 16, K rows written 4 K), + 8 K n with
      --feedback (the residual read and written);
  (b) ga_diloco_outer with momentum on the same rows, (8 K + 16) n bytes: the
      unquantised fused step;
  (c) ga_stream_copy moving the bytes of (a) (half read, half written): what the box
      streams in the same process.

With every node in one process there is no wire: (a) simulates the numerics of a
quantised exchange and moves more bytes than (b).  One JSON line per case, appended
to --out.

    python tools/time_outer_quant.py [--reps 20] [--pairs 5] [--ks 1,8] [--feedback] [--out profiles/...txt]
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
from gym_amd.engine import DiLoCoOuterQuant  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--ks", default="1,8")
    ap.add_argument("--bits", default="8,4")
    ap.add_argument("--feedback", action="store_true")
    ap.add_argument("--model", default="gpt2-124m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outer_quant.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_outer_quant: no GPU (there is nothing to time on the CPU)")
    dev = torch.device("cuda:0")
    n = ArenaLayout(MODELS[a.model]()).n
    coll = Collective()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for K in [int(k) for k in a.ks.split(",")]:
        for bits in [int(b) for b in a.bits.split(",")]:
            reps = torch.empty(K, n, device=dev)
            for k in range(K):
                reps[k].normal_(std=0.02)
            eng = DiLoCoOuterQuant(coll, K, n, dev, torch.float32, bits=bits, error_feedback=a.feedback, **SGD)
            eng.init_master(reps[0])
            eng.first = False
            sgd_master, sgd_mom = reps[0].clone(), torch.zeros(n, device=dev)
            b = bits / 8 + 1 / 64
            bytes_a = int((20 + K * (8 + 2 * b) + (8 * K if a.feedback else 0)) * n)
            bytes_b = (8 * K + 16) * n
            half = (bytes_a // 2 + 15) // 16 * 16
            src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8,
                                                                                      device=dev)

            out = torch.empty_like(reps)

            def quant():  # the engine's two launches, the new rows to a second set so the deltas stay non-zero
                ops.quant_encode(reps, eng.master, eng.residual, eng.payload, n, bits)
                ops.diloco_outer_dequant(eng.payload, eng.master, eng.mom, out, n, bits, K, SGD["lr"],
                                         SGD["momentum"], SGD["dampening"], SGD["weight_decay"], SGD["nesterov"],
                                         False)

            def encode():
                ops.quant_encode(reps, eng.master, eng.residual, eng.payload, n, bits)

            def sgd():
                ops.diloco_outer(reps, sgd_master, sgd_mom, reps, n, K, SGD["lr"], SGD["momentum"], SGD["dampening"],
                                 SGD["weight_decay"], SGD["nesterov"], False)

            def copy():
                ops.stream_copy(src, dst)

            rounds = [(timed(quant, a.reps), timed(sgd, a.reps), timed(copy, a.reps), timed(encode, a.reps))
                      for _ in range(a.pairs)]
            ms_a, ms_b, ms_c, ms_e = (sum(r[i] for r in rounds) / len(rounds) for i in range(4))
            line = json.dumps({
                "what": "DiLoCo outer step on block-quantised pseudo-gradients", "model": a.model, "K": K, "n": n,
                "bits": bits, "error_feedback": a.feedback, "reps": a.reps,
                "payload_bytes_per_node": eng.payload_bytes_per_node,
                "quant_ms": round(ms_a, 4), "encode_ms": round(ms_e, 4), "decode_ms": round(ms_a - ms_e, 4),
                "sgd_outer_ms": round(ms_b, 4), "copy_ms": round(ms_c, 4),
                "rounds_ms_quant_sgd_copy_encode": [[round(x, 4) for x in r] for r in rounds],
                "quant_bytes": bytes_a, "quant_bytes_per_elem": round(bytes_a / n, 2),
                "quant_frac_of_8TBps": round(bytes_a / (ms_a * 1e-3) / PEAK, 4),
                "sgd_outer_bytes": bytes_b, "sgd_outer_frac_of_8TBps": round(bytes_b / (ms_b * 1e-3) / PEAK, 4),
                "copy_bytes": 2 * half, "copy_frac_of_8TBps": round(2 * half / (ms_c * 1e-3) / PEAK, 4),
                "quant_over_copy": round(ms_a / ms_c, 3), "quant_over_sgd_outer": round(ms_a / ms_b, 3),
            })
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
            del reps, out, eng, sgd_master, sgd_mom, src, dst
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
