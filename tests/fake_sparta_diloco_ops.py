"""CPU stand-in for gym_amd.ops.diloco_outer_masked — TEST INFRASTRUCTURE.

install() installs tests/fake_ops.py and adds the masked outer step as what it
replaces: fake_ops.sparta_average_local then fake_ops.diloco_outer on the same
buffers.  This covers the Python plumbing only (which step takes the one-pass
path, with which mask and divisors); the kernel's own arithmetic is pinned on
the GPU against the two real kernels (tests/test_gpu_sparta_diloco.py).
"""
import fake_ops

CALLS = []  # (n, selected count) of every masked outer step, for the tests that ask which path ran


def diloco_outer_masked(reps, bits, master, mom, n, sparse_divisor, divisor, lr, momentum, dampening, weight_decay,
                        nesterov, first_step):
    CALLS.append((int(n), int(fake_ops._mask_bits(bits, n).sum())))
    fake_ops.sparta_average_local(reps, n, sparse_divisor, mask=bits)
    fake_ops.diloco_outer(reps, master, mom, reps, n, divisor, lr, momentum, dampening, weight_decay, nesterov,
                          first_step)


def install():
    fake_ops.install()
    fake_ops.diloco_outer_masked = diloco_outer_masked
