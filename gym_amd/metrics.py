"""Node drift: how far the simulated nodes' models are apart.

The reference's model-correlation metric (exogym/train_node.py:498-573, called
from :614-616) saves every node's state dict to disk, loads them all on rank 0
and runs np.corrcoef on each pair; it is disabled there by a leading `return`.
Here the nodes' parameters already sit in [K, ld] arenas, so the metric is one
read of them: ga_replica_gram gives the K x K Gram matrix, the row sums and each
node's squared distance to the node mean, and the rest is K x K host arithmetic
in float64.
"""
import numpy as np
import torch

from . import ops

MAX_NODES = 32  # ga_replica_gram's limit


def correlation_from_gram(gram, rowsum, n_true):
    """The [K, K] Pearson correlation matrix of K vectors of n_true elements from
    their Gram matrix G and sums s, in float64 on the host:
    cov_ij = G_ij - s_i s_j / n_true, corr_ij = cov_ij / sqrt(cov_ii cov_jj).
    A vector of zero variance gives NaN in its row and column, as np.corrcoef
    does.  Zero padding beyond n_true adds nothing to G or s."""
    G = np.asarray(gram, dtype=np.float64)
    s = np.asarray(rowsum, dtype=np.float64)
    cov = G - np.outer(s, s) / float(n_true)
    var = np.diag(cov).copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        corr = cov / np.sqrt(np.outer(var, var))
        corr[var <= 0.0, :] = np.nan
        corr[:, var <= 0.0] = np.nan
    return np.clip(corr, -1.0, 1.0)  # as np.corrcoef clips; NaN stays NaN


def drift_summary(gram, rowsum, dist2, n_true):
    """The dict NodeDrift returns, from host copies of the kernel's outputs."""
    G = np.asarray(gram, dtype=np.float64)
    d2 = np.asarray(dist2, dtype=np.float64)
    corr = correlation_from_gram(G, rowsum, n_true)
    iu = np.triu_indices(G.shape[0], k=1)
    return {
        "correlation": corr.tolist(),
        "avg_model_correlation": float(np.mean(corr[iu])),
        "norm": np.sqrt(np.diag(G)).tolist(),
        "dist_to_mean": np.sqrt(d2).tolist(),
        "consensus_distance": float(np.mean(d2)),
    }


class NodeDrift:
    """Model correlation and consensus distance over all simulated nodes.

    coll: this process's Collective; K_local: nodes hosted by this process (its
    rows are nodes rank * K_local ...); ld: row length of the arena; n: elements
    of a row the kernel covers; n_true: real parameters (sum of the layout's
    numels; the alignment padding inside [0, n) is zero and adds nothing).

    __call__(P) takes this process's [K_local, ld] rows (a 1-D [ld] arena for
    K_local = 1) and is called by EVERY rank.  At world size 1 the kernel runs on
    P; otherwise one all-gather into a lazily allocated [num_nodes, ld] buffer in
    node order, then the kernel on rank 0 only.  Rank 0 gets

      correlation            [K][K] Pearson correlations of the parameter vectors
      avg_model_correlation  mean over i < j: the reference's logged number
      norm                   |x_k|
      dist_to_mean           |x_k - mean_k x_k|
      consensus_distance     mean_k |x_k - mean x|^2

    every other rank None.  The vector is the parameter arena; the reference
    concatenates the sorted state dict, which also holds buffers (BatchNorm
    statistics, step counters).  Pearson correlation does not depend on the
    element order, so the two agree for a model without buffers.
    """

    def __init__(self, coll, K_local, ld, n, n_true, device, dtype):
        self.coll = coll
        self.K_local = int(K_local)
        self.num_nodes = coll.world * self.K_local
        if self.num_nodes < 2:
            raise Exception("Correlation calculation cannot be used with < 2 nodes")
        if self.num_nodes > MAX_NODES:
            raise ValueError(f"NodeDrift: {self.num_nodes} nodes, the Gram kernel supports at most {MAX_NODES}")
        self.ld, self.n, self.n_true = int(ld), int(n), int(n_true)
        if not 0 < self.n_true <= self.n <= self.ld:
            raise ValueError(f"NodeDrift: need 0 < n_true <= n <= ld, got {n_true}, {n}, {ld}")
        self.device, self.dtype = device, dtype
        self._all = None  # [num_nodes, ld], allocated at the first multi-process call

    @torch.no_grad()
    def __call__(self, P):
        P = P.detach().view(self.K_local, -1) if P.dim() == 1 else P.detach()
        if tuple(P.shape) != (self.K_local, self.ld):
            raise ValueError(f"NodeDrift: expected rows of shape {(self.K_local, self.ld)}, got {tuple(P.shape)}")
        src = P
        if self.coll.exchange:
            if self._all is None:
                self._all = torch.empty(self.num_nodes, self.ld, device=self.device, dtype=self.dtype)
            self.coll.all_gather_into(self._all.view(-1), P.reshape(-1))
            if self.coll.rank != 0:
                return None
            src = self._all
        gram, rowsum, dist2 = ops.replica_gram(src, n=self.n, want_dist=True)
        return drift_summary(gram.cpu().numpy(), rowsum.cpu().numpy(), dist2.cpu().numpy(), self.n_true)


def flat_parameters(model):
    """One node's parameters as a flat vector (a strategy without an arena): a
    copy, built per measurement.  Returns (flat, n_true)."""
    ps = [p.detach().reshape(-1) for p in model.parameters()]
    flat = torch.cat(ps)
    return flat, flat.numel()


__all__ = ["NodeDrift", "correlation_from_gram", "drift_summary", "flat_parameters", "MAX_NODES"]
