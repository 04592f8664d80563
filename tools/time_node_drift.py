"""Time ga_replica_gram (the node-drift metric's kernel) over GPT-2 124M rows at
K = 8 and K = 32 replicas beside ga_stream_copy of the same bytes in the same
process: queued back-to-back launches between two device events.  Prints one JSON
line per K: milliseconds per launch, the bytes the kernel reads over that time as
a fraction of 8 TB/s, and the copy's figures (a copy moves the bytes twice).
A second line per K times ga_replica_gram_centered (drift_detail=True) on the same
rows, alternated with ga_replica_gram with dist2, and gives the ratio of the two.

    python tools/time_node_drift.py [--reps 20] [--ks 8,32] [--dtype fp32|bf16]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_amd import _lib, ops  # noqa: E402
from gym_amd.arena import ArenaLayout  # noqa: E402
from gym_amd.shapes import MODELS  # noqa: E402

PEAK = 8e12  # B/s, MI355X HBM3E


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
    ap.add_argument("--ks", default="8,32")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--model", default="gpt2-124m")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_node_drift: no GPU (there is nothing to time on the CPU)")
    dev = torch.device("cuda:0")
    dt = torch.float32 if a.dtype == "fp32" else torch.bfloat16
    ld = ArenaLayout(MODELS[a.model]()).n
    L = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for K in [int(k) for k in a.ks.split(",")]:
        src = torch.empty(K, ld, device=dev, dtype=dt)
        for k in range(K):
            src[k].normal_()
        nbytes = src.numel() * src.element_size()
        gram = torch.empty(K, K, dtype=torch.float64, device=dev)
        rowsum = torch.empty(K, dtype=torch.float64, device=dev)
        dist2 = torch.empty(K, dtype=torch.float64, device=dev)
        work = torch.empty(L.ga_replica_gram_workspace_bytes(K, ld) // 4, dtype=torch.float32, device=dev)
        code = _lib.GA_F32 if dt == torch.float32 else _lib.GA_BF16

        def run(d2):
            _lib.check(L.ga_replica_gram(code, src.data_ptr(), K, ld, ld, gram.data_ptr(), rowsum.data_ptr(),
                                         d2.data_ptr() if d2 is not None else None, work.data_ptr(), stream),
                       "ga_replica_gram")

        cgram = torch.empty(K, K, dtype=torch.float64, device=dev)
        mdot = torch.empty(K, dtype=torch.float64, device=dev)
        dsum = torch.empty(K, dtype=torch.float64, device=dev)
        mstat = torch.empty(2, dtype=torch.float64, device=dev)
        cwork = torch.empty(L.ga_replica_gram_centered_workspace_bytes(K, ld) // 4, dtype=torch.float32, device=dev)

        def run_centered():
            _lib.check(L.ga_replica_gram_centered(code, src.data_ptr(), K, ld, ld, cgram.data_ptr(), mdot.data_ptr(),
                                                  dsum.data_ptr(), mstat.data_ptr(), cwork.data_ptr(), stream),
                       "ga_replica_gram_centered")

        ms = timed(lambda: run(dist2), a.reps)
        ms_nodist = timed(lambda: run(None), a.reps)
        dst = torch.empty_like(src)
        ms_copy = timed(lambda: ops.stream_copy(src.view(-1), dst.view(-1)), a.reps)
        del dst
        print(json.dumps({
            "kernel": "ga_replica_gram", "model": a.model, "dtype": a.dtype, "K": K, "ld": ld, "bytes_read": nbytes,
            "ms": round(ms, 4), "frac_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK, 4),
            "ms_without_dist2": round(ms_nodist, 4),
            "stream_copy_ms": round(ms_copy, 4),
            "stream_copy_frac_of_8TBps": round(2 * nbytes / (ms_copy * 1e-3) / PEAK, 4),
            "gram_ms_over_copy_ms": round(ms / ms_copy, 3),
        }), flush=True)
        # the two kernels alternated on the same rows: the spread of the rounds is the noise
        rounds = [(timed(lambda: run(dist2), a.reps), timed(run_centered, a.reps)) for _ in range(3)]
        ms_plain = sum(r[0] for r in rounds) / len(rounds)
        ms_cen = sum(r[1] for r in rounds) / len(rounds)
        print(json.dumps({
            "kernel": "ga_replica_gram_centered", "model": a.model, "dtype": a.dtype, "K": K, "ld": ld,
            "bytes_read": nbytes, "ms": round(ms_cen, 4), "frac_of_8TBps": round(nbytes / (ms_cen * 1e-3) / PEAK, 4),
            "gram_with_dist2_ms": round(ms_plain, 4), "centered_ms_over_gram_ms": round(ms_cen / ms_plain, 3),
            "rounds_ms_gram_centered": [[round(p, 4), round(c, 4)] for p, c in rounds],
            "stream_copy_ms": round(ms_copy, 4), "centered_ms_over_copy_ms": round(ms_cen / ms_copy, 3),
        }), flush=True)
        del src, work, cwork


if __name__ == "__main__":
    main()
