"""Fused inner optimizer on the MI355X (ga_adam_step, ga_grad_clip_coef through
the C ABI) against torch.optim.AdamW / Adam + clip_grad_norm_ running on the
same GPU (the reference's inner optimizer).  fp32 tolerance: reordered norm
sums and FMA contraction differ at the ulp level; 1e-5 relative after 5 steps.

With a presence pattern (optim_cases.Pattern) the kernel runs over ranges of
the arena; after every step the sentinels check what it must not have touched:
the padding of the parameter / gradient / moment rows, the absent tensors'
spans, and 64 elements behind each row."""
import pytest
import torch

import optim_cases as C

pytestmark = pytest.mark.gpu

GUARD = 64


def sentinels(max_norm):
    """An observer for optim_cases.run_pair on the GPU.  Before each step it
    snapshots the four sets; after it, every element outside the present
    tensors' spans must be bit-identical in the parameters and both moments
    (the padding, the absent and frozen tensors, the 64 elements behind each row
    where the storage has them) and zero in the gradients; and with clipping the
    present tensors' gradients are bitwise g * coef, coef read back from the
    device (exactly g when the kernel does not scale: coef >= 1)."""
    snap = {}

    def rows(opt):
        """Each row with the GUARD elements behind it: the head of the next row,
        or for the last row what its storage holds behind it (run_pair's `slack`
        puts all four sets into buffers with GUARD elements to spare)."""
        out = {}
        for name, rs in (("param", list(opt.P.unbind(0))), ("grad", list(opt.G.unbind(0))),
                         ("exp_avg", opt._Mr), ("exp_avg_sq", opt._Vr)):
            last, s = rs[-1], rs[-1].untyped_storage()
            have = (s.nbytes() - (last.data_ptr() - s.data_ptr())) // 4 - last.numel()
            tail = torch.as_strided(last, (max(0, min(GUARD, have)),), (1,), last.storage_offset() + last.numel())
            out[name] = [torch.cat([r, nxt[:GUARD]]) for r, nxt in zip(rs, rs[1:] + [tail])]
        return out

    def observe(when, step, ctx):
        opt = ctx["opt"]
        if when == "before":
            snap.clear()
            snap.update({name: [r.clone() for r in rs] for name, rs in rows(opt).items()})
            return
        now = rows(opt)
        spans = []
        for pat, ar in zip(ctx["pats"], opt.arenas):
            L = ar.layout
            spans.append([(o, n) for i, (o, n) in enumerate(zip(L.offsets, L.numels)) if pat.present(i, step)])
        for k in range(opt.K):
            keep = torch.ones(now["param"][k].numel(), dtype=torch.bool, device=opt.P.device)
            for o, n in spans[k]:
                keep[o:o + n] = False
            for o, n in (spans[k + 1] if k + 1 < opt.K else []):  # the next row's head is behind this row
                keep[opt.ld + o:opt.ld + min(o + n, GUARD)] = False
            live = ~keep[:opt.ld]
            for name in ("param", "exp_avg", "exp_avg_sq"):
                assert now[name][k].numel() == opt.ld + GUARD  # the guard is there, for the last row too
                a, b = snap[name][k][keep], now[name][k][keep]
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                    f"step {step} replica {k}: {name} changed outside the present tensors"
            g0, g1 = snap["grad"][k], now["grad"][k]
            assert torch.equal(g0[keep].view(torch.int32), g1[keep].view(torch.int32))
            assert not bool(g1[:opt.ld][~live].any()), f"step {step} replica {k}: an absent gradient span is not zero"
            if max_norm and spans[k]:
                coef = opt._clip[2 * k]
                want = g0[:opt.ld][live] if bool(coef >= 1.0) else g0[:opt.ld][live] * coef
                assert torch.equal(want.view(torch.int32), g1[:opt.ld][live].view(torch.int32)), \
                    f"step {step} replica {k}: present gradients are not g * coef"
            else:
                assert torch.equal(g0[:opt.ld].view(torch.int32), g1[:opt.ld].view(torch.int32))

    return observe


@pytest.mark.parametrize("name,cls,kw,max_norm,skip,pattern", C.CASES, ids=[c[0] for c in C.CASES])
def test_arena_adam_matches_torch_on_gpu(name, cls, kw, max_norm, skip, pattern):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ours, ref = C.run_pair("cuda:0", cls, kw, max_norm=max_norm, skip=skip, pattern=pattern,
                           steps=C.case_steps(pattern), observe=sentinels(max_norm), slack=GUARD)
    C.assert_close(ours, ref)


@pytest.mark.parametrize("name,cls,kw,max_norm", C.REPLICA_CASES, ids=[c[0] for c in C.REPLICA_CASES])
def test_arena_adam_replicas_match_torch_on_gpu(name, cls, kw, max_norm):
    """K = 3 rows of a ReplicaArena, a different presence pattern on each (the
    ranges, the clip[2k:2k+2] slices and the counts differ per row), against
    three independent torch optimizers on the same GPU."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ours, ref = C.run_pair("cuda:0", cls, kw, max_norm=max_norm, pattern=C.REPLICA_PATTERNS, K=3,
                           steps=C.PATTERN_STEPS, observe=sentinels(max_norm), slack=GUARD)
    C.assert_close(ours, ref)


def test_clip_coef_kernel():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gym_amd import ops
    g = torch.randn(1_000_003, device="cuda") * 0.01
    part, out = ops.sumsq_partials(g.device), torch.zeros(2, device="cuda")
    ops.grad_clip_coef(g, g.numel(), 0.5, part, out)
    ref = torch.linalg.vector_norm(g.double()).item()
    assert abs(out[1].item() - ref) <= 1e-5 * ref
    assert abs(out[0].item() - min(1.0, 0.5 / (ref + 1e-6))) <= 1e-5
