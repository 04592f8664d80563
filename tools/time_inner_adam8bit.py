"""Time the fused 8-bit AdamW inner step (ga_adam8_step through gym_amd.fused_optim.ArenaAdam8bit) on
GPT-2 124M rows at K = 1 and K = 8, in alternated pairs against three things in the same process:
ga_adam_step (ArenaAdam, its moments left where they are allocated: no placement search) on the same
rows, the torch class AdamW8bit (one optimizer per replica, as replica._PerNodeOptim builds them), and
a ga_stream_copy that moves as many bytes as the step (16.25 B per element: p read and written, g
read, two code bytes read and written, two scales per 64 elements read and written).  Beside the
times: the optimizer state each side allocated.

Every timed window holds about WINDOW_S of queued work (the repetitions are sized from a first
estimate), after a warm-up of the same launches.

    python tools/time_inner_adam8bit.py > profiles/inner_adam8bit.txt
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_amd import ops, shapes  # noqa: E402
from gym_amd.arena import ReplicaArena  # noqa: E402
from gym_amd.fused_optim import ArenaAdam, ArenaAdam8bit  # noqa: E402
from gym_amd.strategy.optim import AdamW8bit  # noqa: E402

WINDOW_S = 0.3
BYTES_8BIT, BYTES_FP32 = 16.25, 28.0  # per element and step


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
    print(f"# {a.model}: {len(shape_list)} tensors, {torch.cuda.get_device_name(0)}")
    for K in a.K:
        torch.manual_seed(0)
        models = [Bag(shape_list, dev) for _ in range(K)]
        ra = ReplicaArena(models)
        n = K * ra.ld
        fused = ArenaAdam8bit(ra.params, ra)
        fp32 = ArenaAdam(ra.params, ra, placement=False)
        plain = [AdamW8bit(list(m.parameters())) for m in models]
        ra.grad_set.normal_(0, 1e-2)
        for ar in ra.arenas:
            ar.rebind_grads()
        src = torch.empty(int(n * BYTES_8BIT / 8), dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)

        def unfused():
            for o in plain:
                o.step()

        others = (("ga_adam_step", fp32.step), ("AdamW8bit (torch)", unfused),
                  ("copy of its bytes", lambda: ops.stream_copy(src, dst)))
        for fn in (fused.step, fp32.step, unfused):  # warm-up: tables, kernels, state
            fn()
        torch.cuda.synchronize()
        plain_bytes = sum(v.numel() * v.element_size() for o in plain for st in o.state.values()
                          for v in st.values() if torch.is_tensor(v) and v.is_cuda)
        print(f"K={K} ld={ra.ld} state: ArenaAdam8bit {fused.state_bytes() / 2**20:.1f} MiB "
              f"({fused.state_bytes() / n:.3f} B per element), AdamW8bit (torch) {plain_bytes / 2**20:.1f} MiB, "
              f"ArenaAdam {2 * n * 4 / 2**20:.1f} MiB (8 B per element)")
        for name, fn in others:
            pairs = [(window(fused.step), window(fn)) for _ in range(a.pairs)]
            for f, u in pairs:
                print(f"  pair: ga_adam8_step {f:9.3f} ms   {name} {u:9.3f} ms   ratio {u / f:6.2f}x")
            print(f"  ga_adam8_step faster than {name} in every pair: {all(f < u for f, u in pairs)}")
        f = min(window(fused.step) for _ in range(3))
        g = min(window(fp32.step) for _ in range(3))
        print(f"  best of 3: ga_adam8_step {f:.3f} ms = {n / f / 1e6:.1f} G elements/s, {n * BYTES_8BIT / f / 1e9:.2f} TB/s "
              f"of its {BYTES_8BIT} B; ga_adam_step {g:.3f} ms = {n / g / 1e6:.1f} G elements/s, "
              f"{n * BYTES_FP32 / g / 1e9:.2f} TB/s of its {BYTES_FP32:.0f} B")
        del fused, fp32, plain, ra, models, src, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
