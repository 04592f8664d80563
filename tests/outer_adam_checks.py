"""References for one Adam outer step from a given pre-state -- TEST INFRASTRUCTURE.

Adam's update is m / sqrt(v), sign-like where |g| is tiny: an ulp of difference
in g there becomes a difference of order lr one step later.  So every check
here is ONE outer step from a state that was read back (master, exp_avg,
exp_avg_sq, t), never a trajectory: restarted like that the oracle is within
0.08x of rtol 1e-5 / atol 1e-7 of torch.optim.Adam / AdamW on the master and
bit-identical on the moments (n = 8340, lr 0.05, K in {1, 3, 8}, 4 steps, CPU).
"""
import numpy as np
import torch

from oracle import optim as ooptim
from oracle import reduce as oreduce

P_TOL = dict(rtol=1e-5, atol=1e-7)  # master: check_adam_replica's, tests/sgd_kernel_checks.py
M_TOL = dict(rtol=1e-6, atol=0)     # exp_avg / exp_avg_sq


def oracle_step(rows, divisor, master, m, v, t, hp):
    """(master, exp_avg, exp_avg_sq) after outer step t (the count after the
    increment) from numpy fp32 pre-state: oracle.reduce.mean_reduce over the rows
    (bf16 rows widened to fp32 by the caller), an fp32 subtract, oracle.optim.adam_step.
    hp: lr, betas, eps, weight_decay, decoupled."""
    avg = oreduce.mean_reduce(list(rows), divisor=divisor)
    g = (np.asarray(master, np.float32) - avg).astype(np.float32)
    p, _, m2, v2 = ooptim.adam_step(master, g, m, v, t, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"],
                                    weight_decay=hp["weight_decay"], decoupled=hp["decoupled"])
    return p, m2, v2


def torch_step(cls, kwargs, master, m, v, t_before, avg):
    """The same step by torch's optimizer `cls(**kwargs)` loaded with the pre-state
    (tensors on any device; t_before = steps already taken): master.grad = master
    - avg as DiLoCoStrategy._outer_step forms it.  Returns numpy (master, m, v)."""
    p = torch.nn.Parameter(master.detach().clone())
    opt = cls([p], **kwargs)
    opt.state[p] = {"step": torch.tensor(float(t_before)), "exp_avg": m.detach().clone(),
                    "exp_avg_sq": v.detach().clone()}
    p.grad = p.detach() - avg.float()
    opt.step()
    st = opt.state[p]
    return tuple(x.detach().cpu().numpy() for x in (p, st["exp_avg"], st["exp_avg_sq"]))


def assert_step(got, want, what=""):
    """got / want: (master, exp_avg, exp_avg_sq) numpy arrays."""
    np.testing.assert_allclose(got[0], want[0], err_msg=f"{what} master", **P_TOL)
    np.testing.assert_allclose(got[1], want[1], err_msg=f"{what} exp_avg", **M_TOL)
    np.testing.assert_allclose(got[2], want[2], err_msg=f"{what} exp_avg_sq", **M_TOL)


def bit_shares(got, want):
    """Share of bit-identical elements per (master, exp_avg, exp_avg_sq)."""
    return tuple(float(np.mean(np.asarray(a).view(np.uint32) == np.asarray(b).view(np.uint32)))
                 for a, b in zip(got, want))
