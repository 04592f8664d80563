"""Numpy stand-in for gym_amd.ops.replica_gram (CPU tests of gym_amd.metrics):
the definitions of include/gym_amd.h in float64, on CPU tensors."""
import types

import numpy as np
import torch


def reference(x):
    """(gram, rowsum, dist2) of the rows of a float64 [K, n] array."""
    x = np.asarray(x, dtype=np.float64)
    c = x - x.mean(axis=0, keepdims=True)
    return x @ x.T, x.sum(axis=1), (c * c).sum(axis=1)


def replica_gram(src, n=None, want_dist=True):
    src2 = src if src.dim() == 2 else src.view(1, -1)
    n = src2.shape[1] if n is None else int(n)
    gram, rowsum, dist2 = reference(src2[:, :n].detach().cpu().double().numpy())
    return torch.from_numpy(gram), torch.from_numpy(rowsum), (torch.from_numpy(dist2) if want_dist else None)


def rank_rows(rank, K_local, ld, n, n_true):
    """The [K_local, ld] float32 rows a rank of the gloo test holds: seeded per
    rank, zero in the padding [n_true, n), junk beyond n."""
    g = torch.Generator().manual_seed(1000 + rank)
    P = torch.randn(K_local, ld, generator=g) + 0.25 * rank
    P[:, n_true:n] = 0.0
    P[:, n:] = 1e30
    return P


def drift_worker(rank, world, port, K_local, ld, n, n_true, out_dir):
    """One process of a gloo world: NodeDrift over the stand-in, result as JSON."""
    import json
    import os

    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    install()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gym_amd.comm import Collective
        from gym_amd.metrics import NodeDrift
        drift = NodeDrift(Collective(), K_local, ld, n, n_true, torch.device("cpu"), torch.float32)
        out = drift(rank_rows(rank, K_local, ld, n, n_true))
        with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
            json.dump(out, f)
    finally:
        dist.destroy_process_group()


def install():
    """Point gym_amd.metrics at the stand-in (this process only)."""
    import gym_amd.metrics as metrics
    metrics.ops = types.SimpleNamespace(replica_gram=replica_gram)
