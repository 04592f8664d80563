"""The host plan of the low-rank (PowerSGD) outer step: which tensors of an arena are
compressed at rank r, where their factors live, and the job lists of the four kernels of
csrc/lowrank.hip (include/gym_amd.h "DiLoCo outer step on low-rank pseudo-gradients").

A tensor of shape (d0, ..) is the m x n matrix d0 x numel / d0; it is compressed iff
ndim >= 2 and r (m + n) < m n.  Everything else -- 1-D tensors, matrices too small to gain,
padding -- is dense and covered by segments.  Buffers:

  A  [a_len]  the m_t x r factors P_t, then (from a multiple of 4) the dense segments' sums
  B  [b_len]  the n_t x r factors (B_t of a step, Q_t = B_t / K_total the next warm start)

Both are all-reduced whole: wire_floats = a_len + b_len per outer step, flat in the world size.
"""
import numpy as np
import torch

RANK_MAX = 32   # the 32 x 32 MFMA tile of ga_lowrank_project / ga_lowrank_backproject
BAND = 32       # rows (project, outer) or columns (back-project) of a job
OUT_COLS = 128  # columns of an outer job
CHUNK = 4096    # elements of a dense job


def check_rank(r):
    """outer_rank as an int; ValueError unless it is an integer in 1..RANK_MAX."""
    if isinstance(r, bool) or not isinstance(r, int) or not 1 <= r <= RANK_MAX:
        raise ValueError(f"outer_rank={r!r}: expected an integer with 1 <= outer_rank <= {RANK_MAX}")
    return int(r)


def check_lowrank_seed(seed):
    """outer_lowrank_seed as an int; ValueError unless it is an integer in 0..2^63 - 1."""
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 63:
        raise ValueError(f"outer_lowrank_seed={seed!r}: expected an integer with 0 <= outer_lowrank_seed < 2^63")
    return int(seed)


def _up(x, m):
    return -(-x // m) * m


class LowRankPlan:
    def __init__(self, shapes, offsets, n, rank):
        r = self.rank = check_rank(rank)
        self.n = int(n)
        rows, end = [], 0
        for shape, off in zip(shapes, offsets):
            numel = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
            if off % 4 or off < end or off + numel > self.n:
                raise ValueError(f"LowRankPlan: tensor at offset {off} (numel {numel}) is not 4-aligned, overlaps its "
                                 f"predecessor or passes the arena's {self.n} elements")
            end = off + numel
            m = int(shape[0]) if len(shape) >= 2 else 1
            nn = numel // m if m else 0
            kind = int(len(shape) >= 2 and numel > 0 and r * (m + nn) < m * nn)
            rows.append([int(off), m, nn, kind, 0, 0])
        self.tensors = np.array(rows, dtype=np.int64).reshape(-1, 6)
        comp = self.tensors[:, 3] == 1
        self.compressed = [int(t) for t in np.flatnonzero(comp)]
        mr, nr = self.tensors[:, 1] * r * comp, self.tensors[:, 2] * r * comp
        self.tensors[:, 4] = np.cumsum(mr) - mr
        self.tensors[:, 5] = np.cumsum(nr) - nr
        self.p_len, self.b_len = int(mr.sum()), int(nr.sum())
        # dense segments: the arena less the compressed tensors, from 4-aligned starts
        segs, cur, aoff = [], 0, _up(self.p_len, 4)
        for t in self.compressed + [None]:
            stop = self.n if t is None else int(self.tensors[t, 0])
            if stop > cur:
                segs.append([cur, stop - cur, aoff])
                aoff += _up(stop - cur, 4)
            if t is not None:
                cur = min(_up(stop + int(self.tensors[t, 1] * self.tensors[t, 2]), 4), self.n)
        self.segments = np.array(segs, dtype=np.int64).reshape(-1, 3)
        self.a_len = aoff
        self.wire_floats = self.a_len + self.b_len
        self.wire_bytes = 4 * self.wire_floats

        def jobs(per_tensor, dense):
            out = [(t, b, tile, 0) for t in self.compressed for b, tile in per_tensor(*map(int, self.tensors[t, 1:3]))]
            if dense:
                out += [(-1 - s, c, 0, 0) for s, seg in enumerate(segs) for c in range(-(-seg[1] // CHUNK))]
            return np.array(out, dtype=np.int32).reshape(-1, 4)
        self.project_jobs = jobs(lambda m, nn: [(b, 0) for b in range(-(-m // BAND))], True)
        self.backproject_jobs = jobs(lambda m, nn: [(b, 0) for b in range(-(-nn // BAND))], False)
        self.outer_jobs = jobs(lambda m, nn: [(b, tl) for b in range(-(-m // BAND)) for tl in range(-(-nn // OUT_COLS))],
                               True)
        self.device = None

    def to(self, device):
        """The tables on `device` (uploaded once); a table without rows keeps one row of zeros
        so that its pointer is valid."""
        def up(a):
            a = a if len(a) else np.zeros((1, a.shape[1]), a.dtype)
            return torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.d_tensors, self.d_segments = up(self.tensors), up(self.segments)
        self.d_project, self.d_backproject, self.d_outer = (up(self.project_jobs), up(self.backproject_jobs),
                                                            up(self.outer_jobs))
        self.device = self.d_tensors.device  # with its index, as a tensor on it reports it
        return self

    def warm_start(self, seed):
        """The replicated Q of the first step: torch.randn on the CPU generator of `seed`, one
        n_t x r draw per compressed tensor in tensor order (identical on every rank)."""
        gen = torch.Generator().manual_seed(check_lowrank_seed(seed))
        q = torch.zeros(max(self.b_len, 1), dtype=torch.float32)
        for t in self.compressed:
            nn, qoff = int(self.tensors[t, 2]), int(self.tensors[t, 5])
            q[qoff:qoff + nn * self.rank] = torch.randn(nn, self.rank, generator=gen, dtype=torch.float32).view(-1)
        return q
