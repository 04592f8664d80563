"""Time DiLoCo's top-k sparse outer step over GPT-2 124M rows, fp32, at K = 1 / 8 / 32
replicas in one process and k = 32 entries per 4096-element chunk, with and without error
feedback: queued back-to-back launches between two device events, the forms taken in
turn for --pairs rounds in one process (the spread of the rounds is the noise):

  encode       ga_topk_encode over the K rows; (4 + K (4 + 6 k / 4096)) n bytes, + 8 K n
               with feedback (the residual read and written);
  decode       ga_diloco_outer_sparse on the K payload rows, the new master to a second
               [K, n] set (so the deltas of the next repetition are not zero);
               (16 + K (4 + 6 k / 4096)) n bytes;
  both         the engine's two launches;
  copy_e/_d    ga_stream_copy moving each kernel's bytes (half read, half written): what
               the box streams in the same process;
  int8         ga_quant_encode + ga_diloco_outer_dequant on the same rows.

With every node in one process there is no wire: this measures the kernels, not the
exchange they shrink.  One JSON line per case, appended to --out.

    python tools/time_outer_topk.py [--reps 20] [--pairs 5] [--ks 1,8,32] [--topk 32] [--out profiles/...txt]
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
from gym_amd.engine import DiLoCoOuterQuant, DiLoCoOuterTopK  # noqa: E402
from gym_amd.shapes import MODELS  # noqa: E402

PEAK = 8e12  # B/s, MI355X HBM3E
SGD = dict(lr=0.7, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=True)
STEP = (SGD["lr"], SGD["momentum"], SGD["dampening"], SGD["weight_decay"], SGD["nesterov"], False)


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


def copier(nbytes, dev):
    half = (nbytes // 2 + 15) // 16 * 16
    src, dst = (torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(2))
    return lambda: ops.stream_copy(src, dst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--topk", type=int, default=32)
    ap.add_argument("--model", default="gpt2-124m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outer_topk.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_outer_topk: no GPU (there is nothing to time on the CPU)")
    dev = torch.device("cuda:0")
    n, k = ArenaLayout(MODELS[a.model]()).n, a.topk
    coll = Collective()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for K in [int(x) for x in a.ks.split(",")]:
        for feedback in (False, True):
            reps = torch.empty(K, n, device=dev)
            for r in range(K):
                reps[r].normal_(std=0.02)
            out = torch.empty_like(reps)
            eng = DiLoCoOuterTopK(coll, K, n, dev, torch.float32, k=k, error_feedback=feedback, **SGD)
            q8 = DiLoCoOuterQuant(coll, K, n, dev, torch.float32, bits=8, error_feedback=feedback, **SGD)
            for e in (eng, q8):
                e.init_master(reps[0])
            pay = 6 * k / 4096
            bytes_e = int((4 + K * (4 + pay) + (8 * K if feedback else 0)) * n)
            bytes_d = int((16 + K * (4 + pay)) * n)

            def encode():
                ops.topk_encode(reps, eng.master, eng.residual, eng.payload, n, k)

            def decode():
                ops.diloco_outer_sparse(eng.payload, eng.master, eng.mom, out, n, k, K, *STEP)

            def both():
                encode()
                decode()

            def int8():
                ops.quant_encode(reps, q8.master, q8.residual, q8.payload, n, 8)
                ops.diloco_outer_dequant(q8.payload, q8.master, q8.mom, out, n, 8, K, *STEP)

            forms = [encode, decode, both, copier(bytes_e, dev), copier(bytes_d, dev), int8]
            rounds = [[timed(f, a.reps) for f in forms] for _ in range(a.pairs)]
            ms_e, ms_d, ms_b, ms_ce, ms_cd, ms_q = (sum(r[i] for r in rounds) / len(rounds) for i in range(6))
            line = json.dumps({
                "what": "DiLoCo outer step on top-k sparse pseudo-gradients", "model": a.model, "K": K, "n": n, "k": k,
                "error_feedback": feedback, "reps": a.reps, "payload_bytes_per_node": eng.payload_bytes_per_node,
                "encode_ms": round(ms_e, 4), "decode_ms": round(ms_d, 4), "both_ms": round(ms_b, 4),
                "copy_encode_bytes_ms": round(ms_ce, 4), "copy_decode_bytes_ms": round(ms_cd, 4),
                "int8_pair_ms": round(ms_q, 4),
                "rounds_ms_encode_decode_both_copye_copyd_int8": [[round(x, 4) for x in r] for r in rounds],
                "encode_bytes": bytes_e, "decode_bytes": bytes_d,
                "encode_frac_of_8TBps": round(bytes_e / (ms_e * 1e-3) / PEAK, 4),
                "decode_frac_of_8TBps": round(bytes_d / (ms_d * 1e-3) / PEAK, 4),
                "encode_over_copy": round(ms_e / ms_ce, 3), "decode_over_copy": round(ms_d / ms_cd, 3),
                "both_over_int8_pair": round(ms_b / ms_q, 3),
            })
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
            del reps, out, eng, q8, forms
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
