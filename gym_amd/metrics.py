"""Node drift: how far the simulated nodes' models are apart.

The reference's model-correlation metric (exogym/train_node.py:498-573, called
from :614-616) saves every node's state dict to disk, loads them all on rank 0
and runs np.corrcoef on each pair; it is disabled there by a leading `return`.
Here the nodes' parameters already sit in [K, ld] arenas, so the metric is one
read of them: ga_replica_gram gives the K x K Gram matrix, the row sums and each
node's squared distance to the node mean, and the rest is K x K host arithmetic
in float64.

detail=True takes the same read through ga_replica_gram_centered instead: the Gram
matrix of the centred values d_k = x_k - mean, with the mean's own sums kept apart,
from which 1 - correlation and the pairwise distances keep their digits when the
nodes are 1e-3 and less apart (np.corrcoef works in float64; an fp32 Gram matrix of
the raw values cancels there).
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


def drift_detail_summary(cgram, mdot, dsum, mstat, n_true):
    """The dict NodeDrift(detail=True) returns, from host copies of
    ga_replica_gram_centered's outputs: C = cgram, b = mdot, t = dsum, A, S = mstat
    (x_k = m + d_k, so G_ij = A + b_i + b_j + C_ij and rowsum_k = S + t_k), all in
    float64 with n = n_true:

      cA = A - S^2/n, cb_k = b_k - S t_k/n, cC_ij = C_ij - t_i t_j/n
      var_k = cA + 2 cb_k + cC_kk, cov_ij = cA + cb_i + cb_j + cC_ij
      1 - corr_ij = num_ij / (r_ij (r_ij + cov_ij)), r_ij = sqrt(var_i var_j)

    where num_ij = var_i var_j - cov_ij^2 is written out with its cA^2 terms
    cancelled on paper, so only terms of the size of the differences remain.  A
    row of zero variance gives NaN in its row and column, as np.corrcoef does.
    The five keys of drift_summary are derived from the same quantities."""
    C = np.asarray(cgram, dtype=np.float64)
    b = np.asarray(mdot, dtype=np.float64)
    t = np.asarray(dsum, dtype=np.float64)
    A, S = (float(v) for v in np.asarray(mstat, dtype=np.float64))
    n = float(n_true)
    K = C.shape[0]
    cA = A - S * S / n
    cb = b - S * t / n
    cC = C - np.outer(t, t) / n
    dg = np.diag(cC).copy()
    var = cA + 2.0 * cb + dg
    cov = cA + cb[:, None] + cb[None, :] + cC
    bi, bj, ci, cj = cb[:, None], cb[None, :], dg[:, None], dg[None, :]
    num = (cA * (ci + cj - 2.0 * cC) - (bi - bj) ** 2 + 2.0 * bi * cj + 2.0 * bj * ci + ci * cj
           - 2.0 * (bi + bj) * cC - cC * cC)
    # var_k is a sum of three rounded terms: a constant row leaves their rounding, not 0
    flat = var <= 64.0 * np.finfo(np.float64).eps * (abs(cA) + 2.0 * np.abs(cb) + np.abs(dg))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(np.outer(var, var))
        omc = np.clip(num / (r * (r + cov)), 0.0, 2.0)  # NaN stays NaN
    omc[flat, :] = np.nan
    omc[:, flat] = np.nan
    corr = 1.0 - omc
    dC = np.diag(C)
    pair = np.sqrt(np.maximum(0.0, dC[:, None] + dC[None, :] - 2.0 * C))
    iu = np.triu_indices(K, k=1)
    return {
        "correlation": corr.tolist(),
        "avg_model_correlation": float(np.mean(corr[iu])),
        "norm": np.sqrt(np.maximum(0.0, A + 2.0 * b + dC)).tolist(),
        "dist_to_mean": np.sqrt(dC).tolist(),
        "consensus_distance": float(np.mean(dC)),
        "one_minus_correlation": omc.tolist(),
        "avg_model_decorrelation": float(np.mean(omc[iu])),
        "pairwise_distance": pair.tolist(),
        "max_pairwise_distance": float(np.max(pair[iu])),
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

    every other rank None.  With detail=True the kernel is ga_replica_gram_centered
    (still one read, after the same all-gather, on rank 0 only) and rank 0 also gets

      one_minus_correlation    [K][K] 1 - correlation, resolved for close nodes
      avg_model_decorrelation  its mean over i < j
      pairwise_distance        [K][K] |x_i - x_j|
      max_pairwise_distance    its maximum

    The vector is the parameter arena; the reference
    concatenates the sorted state dict, which also holds buffers (BatchNorm
    statistics, step counters).  Pearson correlation does not depend on the
    element order, so the two agree for a model without buffers.
    """

    def __init__(self, coll, K_local, ld, n, n_true, device, dtype, detail=False):
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
        self.device, self.dtype, self.detail = device, dtype, bool(detail)
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
        if self.detail:
            out = ops.replica_gram_centered(src, n=self.n)
            return drift_detail_summary(*(o.cpu().numpy() for o in out), self.n_true)
        gram, rowsum, dist2 = ops.replica_gram(src, n=self.n, want_dist=True)
        return drift_summary(gram.cpu().numpy(), rowsum.cpu().numpy(), dist2.cpu().numpy(), self.n_true)


def flat_parameters(model):
    """One node's parameters as a flat vector (a strategy without an arena): a
    copy, built per measurement.  Returns (flat, n_true)."""
    ps = [p.detach().reshape(-1) for p in model.parameters()]
    flat = torch.cat(ps)
    return flat, flat.numel()


__all__ = ["NodeDrift", "correlation_from_gram", "drift_summary", "drift_detail_summary", "flat_parameters",
           "MAX_NODES"]
