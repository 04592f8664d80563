"""Numpy stand-in for gym_amd.ops.replica_gram_centered (CPU tests of
gym_amd.metrics with detail=True): the definitions of include/gym_amd.h with the
node mean m and the centred values d = x - m in float64, on CPU tensors."""
import types

import numpy as np
import torch

import fake_metrics_ops


def reference(x):
    """(cgram, mdot, dsum, mstat) of the rows of a float64 [K, n] array."""
    x = np.asarray(x, dtype=np.float64)
    m = x.sum(axis=0) / x.shape[0]
    d = x - m
    return d @ d.T, d @ m, d.sum(axis=1), np.array([m @ m, m.sum()])


def replica_gram_centered(src, n=None):
    src2 = src if src.dim() == 2 else src.view(1, -1)
    n = src2.shape[1] if n is None else int(n)
    return tuple(torch.from_numpy(np.ascontiguousarray(a))
                 for a in reference(src2[:, :n].detach().cpu().double().numpy()))


def refuse(name):
    def boom(*a, **kw):
        raise AssertionError(f"ops.{name} was called")
    return boom


def install(plain=True, centered=True):
    """Point gym_amd.metrics at both stand-ins (this process only); a kernel switched
    off raises when it is touched."""
    import gym_amd.metrics as metrics
    metrics.ops = types.SimpleNamespace(
        replica_gram=fake_metrics_ops.replica_gram if plain else refuse("replica_gram"),
        replica_gram_centered=replica_gram_centered if centered else refuse("replica_gram_centered"))


def drift_worker(rank, world, port, K_local, ld, n, n_true, out_dir):
    """One process of a gloo world: NodeDrift(detail=True) over the stand-in, result
    as JSON (fake_metrics_ops.drift_worker's rows)."""
    import json
    import os

    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    install(plain=False)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gym_amd.comm import Collective
        from gym_amd.metrics import NodeDrift
        drift = NodeDrift(Collective(), K_local, ld, n, n_true, torch.device("cpu"), torch.float32, detail=True)
        out = drift(fake_metrics_ops.rank_rows(rank, K_local, ld, n, n_true))
        with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
            json.dump(out, f)
    finally:
        dist.destroy_process_group()
