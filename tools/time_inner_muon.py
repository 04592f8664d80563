"""Time the fused Muon inner step (gym_amd.fused_optim.ArenaMuon) on GPT-2 124M rows at K = 1
and K = 8, taken in turn with the unfused step (MuonAdamW: torch.optim.Muon on rocBLAS plus
torch.optim.AdamW, one optimizer per replica as replica._PerNodeOptim builds them) on the same
arena-bound parameters in the same process, alternated pair by pair.

Beside the step: each product kind of an iteration on its own (its nominal FLOPs -- the full
products 2 m^2 n, 2 m^3, 2 m^2 n, although gram and poly compute only the upper tiles -- over its
time, as a fraction of the project's bf16 MFMA roofline, 2516.6 TFLOP/s dense),
and prepare / apply beside a ga_stream_copy that
moves as many bytes (prepare 16 B per element: g, buf read, buf and two bf16 written; apply 10 B).

Every timed window holds about WINDOW_S of queued work (the repetitions are sized from a first
estimate), after a warm-up of the same launches.  The products timed on their own leave the
workspace finite however often they run: gram and poly write A and B from X and A, and the
update runs with alpha = 1, beta = 0 (X' = X; the time of a launch does not depend on the
scalars), so the apply timed after them (lr = 0) reads finite values and leaves the parameters
as they are.

    python tools/time_inner_muon.py > profiles/inner_muon.txt
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_amd import ops, shapes  # noqa: E402
from gym_amd.arena import ReplicaArena  # noqa: E402
from gym_amd.fused_optim import ArenaMuon  # noqa: E402
from gym_amd.strategy.optim import MuonAdamW  # noqa: E402

BF16_PEAK = 2516.6e12
WINDOW_S = 0.3


class Bag(torch.nn.Module):
    def __init__(self, shape_list, dev):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, device=dev) * 0.02) for s in shape_list])


def timed(fn, reps=1):
    """ms per call over one window of `reps` queued calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def window(fn):
    """ms per call over a window of about WINDOW_S, after a warm-up call and a first estimate."""
    fn()
    return timed(fn, max(1, int(WINDOW_S * 1e3 / timed(fn)) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2-124m")
    ap.add_argument("--K", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--pairs", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shape_list = shapes.MODELS[a.model]()
    mask = [len(s) == 2 and i >= 2 for i, s in enumerate(shape_list)]  # not wte (tied with lm_head), not wpe
    print(f"# {a.model}: {sum(mask)} Muon matrices of {len(shape_list)} tensors, {torch.cuda.get_device_name(0)}")
    for K in a.K:
        torch.manual_seed(0)
        models = [Bag(shape_list, dev) for _ in range(K)]
        ra = ReplicaArena(models)
        fused = ArenaMuon(ra.params, ra, mask, placement=False)
        plain = [MuonAdamW(list(m.parameters()), muon_mask=mask) for m in models]
        ra.grad_set.normal_(0, 1e-2)
        for ar in ra.arenas:
            ar.rebind_grads()

        def unfused():
            for o in plain:
                o.step()

        fused.step(), unfused()  # warm-up: tables, rocBLAS handles and kernels
        torch.cuda.synchronize()
        pairs = [(window(fused.step), window(unfused)) for _ in range(a.pairs)]
        print(f"K={K} ld={ra.ld} workspace={fused.workspace.numel() * 2 / 2**20:.1f} MiB "
              f"momentum={fused.B.numel() * 4 / 2**20:.1f} MiB")
        for f, u in pairs:
            print(f"  pair: fused {f:9.3f} ms   unfused {u:9.3f} ms   ratio {u / f:6.2f}x")
        print(f"  fused faster in every pair: {all(f < u for f, u in pairs)}")
        if K != a.K[0]:
            continue
        plan = fused._plan(tuple(range(len(fused._slots))))
        ws = fused.workspace
        m_n = [(min(s[1], s[2]), max(s[1], s[2])) for s in fused._slots]
        flops = {"gram": sum(2 * m * m * n for m, n in m_n), "poly": sum(2 * m ** 3 for m, n in m_n),
                 "update": sum(2 * m * m * n for m, n in m_n)}
        kinds = {"gram": (ops.MUON_GRAM, 1, 0.0, 1.0), "poly": (ops.MUON_POLY, 1, -4.775, 2.0315),
                 "update": (ops.MUON_UPDATE, 2, 1.0, 0.0)}
        for name, (kind, which, al, be) in kinds.items():
            def run():
                for cls in plan.classes:
                    ops.muon_gemm(kind, cls[0], cls[which], plan.mats, ws, 0, al, be)
            ms = min(window(run) for _ in range(3))
            rate = flops[name] / (ms * 1e-3)
            print(f"  {name:6s} {ms:8.3f} ms  {rate / 1e12:8.1f} TFLOP/s nominal  {100 * rate / BF16_PEAK:5.1f}% of bf16 peak")
        n = sum(s[1] * s[2] for s in fused._slots)
        g = fused.param_groups[0]
        prep = lambda: ops.muon_prepare(plan.prep, plan.mats, fused.G[0], fused.B[0], ws, plan.partials,  # noqa: E731
                                        momentum=g["momentum"], one_m_momentum=1 - g["momentum"], nesterov=True)
        app = lambda: ops.muon_apply(plan.prep, plan.mats, fused.P[0], ws, 1, lr=0.0, wd_factor=1.0)  # noqa: E731
        for name, fn, bytes_per in (("prepare", prep, 16), ("apply", app, 10)):
            src = torch.empty(n * bytes_per // 8, dtype=torch.float32, device=dev)
            dst = torch.empty_like(src)
            copy = lambda: ops.stream_copy(src, dst)  # noqa: E731
            t, c = min(window(fn) for _ in range(3)), min(window(copy) for _ in range(3))
            print(f"  {name:7s} {t:8.3f} ms ({n * bytes_per / t / 1e9:6.2f} TB/s)   stream_copy of the same bytes "
                  f"{c:8.3f} ms   {t / c:5.2f}x")
        del src, dst
        del fused, plain, ra, models
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
