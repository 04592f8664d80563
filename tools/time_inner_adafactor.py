"""Time the fused Adafactor inner step (gym_amd.fused_optim.ArenaAdafactor) on GPT-2 124M rows at
K = 1 and K = 8, taken in turn with torch.optim.Adafactor (its default implementation, one
optimizer per replica as replica._PerNodeOptim builds them) on the same arena-bound parameters in
the same process, alternated pair by pair.

Beside the step: each of the three tile kernels on its own beside a ga_stream_copy that moves as
many bytes (stats 8 B per element: g and p read; unorm 4 B: g read; apply 12 B: g and p read, p
written), the two per-tensor kernels, and the bytes of optimizer state each side allocated.

Every timed window holds about WINDOW_S of queued work (the repetitions are sized from a first
estimate), after a warm-up of the same launches.  The kernels timed on their own run at the
optimizer's current count with the tables of a whole step; stats and reduce go on averaging the
same gradient into the state, and the apply timed last moves the parameters as a step would.

    python tools/time_inner_adafactor.py > profiles/inner_adafactor.txt
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_amd import ops, shapes  # noqa: E402
from gym_amd.arena import ReplicaArena  # noqa: E402
from gym_amd.fused_optim import ArenaAdafactor  # noqa: E402

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
    print(f"# {a.model}: {len(shape_list)} tensors, {sum(len(s) == 2 for s in shape_list)} of them matrices, "
          f"{torch.cuda.get_device_name(0)}")
    for K in a.K:
        torch.manual_seed(0)
        models = [Bag(shape_list, dev) for _ in range(K)]
        ra = ReplicaArena(models)
        fused = ArenaAdafactor(ra.params, ra)
        plain = [torch.optim.Adafactor(list(m.parameters())) for m in models]
        ra.grad_set.normal_(0, 1e-2)
        for ar in ra.arenas:
            ar.rebind_grads()

        def unfused():
            for o in plain:
                o.step()

        fused.step(), unfused()  # warm-up: tables and kernels
        torch.cuda.synchronize()
        pairs = [(window(fused.step), window(unfused)) for _ in range(a.pairs)]
        plain_bytes = sum(v.numel() * v.element_size() for o in plain for st in o.state.values()
                          for v in st.values() if torch.is_tensor(v) and v.is_cuda)
        print(f"K={K} ld={ra.ld} state: fused {fused.state_bytes() / 2**20:.3f} MiB (+ {fused._W.numel() * 4 / 2**20:.3f}"
              f" MiB of partials) torch {plain_bytes / 2**20:.3f} MiB; AdamW's two moment sets would be "
              f"{2 * K * ra.ld * 4 / 2**20:.1f} MiB")
        for f, u in pairs:
            print(f"  pair: fused {f:9.3f} ms   torch {u:9.3f} ms   ratio {u / f:6.2f}x")
        print(f"  fused faster in every pair: {all(f < u for f, u in pairs)}")
        plan = fused._plan(tuple(range(len(fused._slots))))
        P, G, S, W = fused.P, fused.G, fused.S, fused._W
        eps1, n = 2.0 ** -23, K * sum(s["rows"] * s["cols"] for s in fused._slots)
        kernels = (
            ("stats", 8, lambda: ops.adafactor_stats(plan.jobs, plan.tens, P, G, S, W, beta2t=0.1)),
            ("reduce", 0, lambda: ops.adafactor_reduce(plan.tens, S, W, beta2t=0.1, rho=0.01, eps1=eps1, eps2=1e-3)),
            ("unorm", 4, lambda: ops.adafactor_unorm(plan.jobs, plan.tens, G, S, W, eps1=eps1)),
            ("scale", 0, lambda: ops.adafactor_scale(plan.tens, W, d=1.0)),
            ("apply", 12, lambda: ops.adafactor_apply(plan.jobs, plan.tens, P, G, S, W, eps1=eps1, wd_factor=1.0)))
        for name, bytes_per, fn in kernels:
            t = min(window(fn) for _ in range(3))
            if not bytes_per:
                print(f"  {name:6s} {t:8.3f} ms (one workgroup per tensor and replica)")
                continue
            src = torch.empty(n * bytes_per // 8, dtype=torch.float32, device=dev)
            dst = torch.empty_like(src)
            c = min(window(lambda: ops.stream_copy(src, dst)) for _ in range(3))
            print(f"  {name:6s} {t:8.3f} ms ({n * bytes_per / t / 1e9:6.2f} TB/s)   stream_copy of the same bytes "
                  f"{c:8.3f} ms   {t / c:5.2f}x")
            del src, dst
        del fused, plain, ra, models, P, G, S, W, plan
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
