"""ga_diloco_outer_masked on the MI355X: bit-identical to ga_sparta_average_local
followed by ga_diloco_outer on every path (vector / scalar, fp32 / bf16, row
padding, K across the unroll boundary, every momentum form, edge masks), and
SPARTADiLoCoStrategy end to end: replica mode fused and not, against a process
per node, through Trainer.fit, and the process-mode composition with an exchange."""
import numpy as np
import pytest
import torch

import replica_scenarios as R
import sparta_diloco_scenarios as SD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_TWO_WG = 4096 * 2 + 64  # two workgroups of the vector path plus a part chunk, a whole number of mask words + 1
N_SCALAR = 4099           # not a multiple of 4: the scalar path, a tail word of 3 bits
N_SMALL = 130             # fewer elements than one chunk, scalar path (130 % 4 != 0)
NS = [N_TWO_WG, N_SCALAR, N_SMALL]
HPS = {
    "nesterov": dict(lr=0.7, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=True),
    "plain": dict(lr=0.3, momentum=0.9, dampening=0.1, weight_decay=0.01, nesterov=False),
    "nomom": dict(lr=0.5, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False),
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _mask(kind, n, g):
    if kind == "random":
        return torch.rand(n, generator=g) < 0.3
    m = torch.zeros(n, dtype=torch.bool)
    if kind == "ones":
        m[:] = True
    elif kind == "last":
        m[n - 1] = True
    return m


def _bits(mask):
    from oracle.sparta import pack_mask
    return torch.from_numpy(pack_mask(mask.numpy())).to(DEV)


def _rows(K, n, ld, dtype, g, misalign):
    """[K, ld] rows of N(0, 1); misalign: a view starting 4 bytes past the
    allocation's 16-byte alignment, which no vector load can take."""
    off = (4 // torch.empty((), dtype=dtype).element_size()) if misalign else 0
    buf = torch.zeros(K * ld + off, dtype=dtype, device=DEV)
    reps = buf[off:].view(K, ld)
    reps.copy_(torch.randn(K, ld, generator=g).to(dtype))
    if misalign:
        assert reps.data_ptr() % 16 == 4
    return reps


def _chain(K, n, pad, dtype, hp_name, mask_kind, sparse_divisor=None, misalign=False, steps=3):
    """Three chained outer steps (first_step true, then false) both ways from the
    same start; the rows drift apart again between the steps.  Returns the
    masked and the two-launch (rows, master, momentum) after every step."""
    from gym_amd import ops
    hp = HPS[hp_name]
    g = torch.Generator().manual_seed(1000 * K + n + pad)
    ld = n + pad
    sd = float(K if sparse_divisor is None else sparse_divisor)
    a = _rows(K, n, ld, dtype, g, misalign)
    b = _rows(K, n, ld, dtype, g, misalign)
    b.copy_(a)
    ma = torch.randn(n, generator=g).to(DEV)
    mb = ma.clone()
    has_mom = hp["momentum"] != 0.0
    va = torch.zeros(n, device=DEV) if has_mom else None
    vb = torch.zeros(n, device=DEV) if has_mom else None
    out = []
    for t in range(steps):
        bits = _bits(_mask(mask_kind, n, g))
        ops.diloco_outer_masked(a[:, :n], bits, ma, va, n, sd, K, hp["lr"], hp["momentum"], hp["dampening"],
                                hp["weight_decay"], hp["nesterov"], t == 0)
        ops.sparta_average_local(b[:, :n], n, sd, mask=bits)
        ops.diloco_outer(b[:, :n], mb, vb, b[:, :n], n, K, hp["lr"], hp["momentum"], hp["dampening"],
                         hp["weight_decay"], hp["nesterov"], t == 0)
        out.append(((a.clone(), ma.clone(), None if va is None else va.clone()),
                    (b.clone(), mb.clone(), None if vb is None else vb.clone())))
        noise = torch.randn(K, ld, generator=g).to(DEV)
        noise[:, n:] = 0
        a.add_(noise.to(dtype))
        b.add_(noise.to(dtype))
    return out


def _cases():
    f32, bf16 = torch.float32, torch.bfloat16
    cs = []
    for dt in (f32, bf16):
        for n in NS:
            for K in (1, 2, 8, 9, 32):                      # 9 crosses the unroll-by-8 boundary
                cs.append((K, n, 0, dt, "nesterov", "random", None, False))
            for K in (8, 9):                                # rows wider than n
                cs.append((K, n, 64, dt, "nesterov", "random", None, False))
            for kind in ("zero", "ones", "last"):
                cs.append((8, n, 0, dt, "nesterov", kind, None, False))
        for n in (N_TWO_WG, N_SCALAR):
            for hp in ("plain", "nomom"):
                cs.append((8, n, 0, dt, hp, "random", None, False))
        for n in (N_TWO_WG, N_SMALL):                       # a vector-sized n that must take the scalar path
            cs.append((8, n, 64, dt, "nesterov", "random", None, True))
        cs.append((8, N_TWO_WG, 0, dt, "nesterov", "random", 24.0, False))  # the two divisors are not confused
        cs.append((32, N_TWO_WG, 64, dt, "plain", "ones", None, False))
    return cs


def _id(c):
    K, n, pad, dt, hp, kind, sd, mis = c
    return f"K{K}-n{n}-pad{pad}-{'f32' if dt == torch.float32 else 'bf16'}-{hp}-{kind}" + \
        (f"-sd{int(sd)}" if sd else "") + ("-misaligned" if mis else "")


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_masked_outer_equals_sparta_then_outer(case):
    _need_gpu()
    K, n, pad, dt, hp, kind, sd, mis = case
    for t, (got, want) in enumerate(_chain(K, n, pad, dt, hp, kind, sd, mis)):
        for name, x, y in zip(("rows", "master", "momentum"), got, want):
            if x is None:
                assert y is None
                continue
            assert torch.equal(x, y), (t, name, int((x != y).sum()))
        rows = got[0]
        assert torch.equal(rows[:, :n], rows[0:1, :n].expand(K, n))  # every row took the master
        assert torch.equal(rows[0, :n].float(), got[1].to(dt).float())
        if pad:
            assert (rows[:, n:] != 0).any() and torch.equal(rows[:, n:], want[0][:, n:])  # the padding is not ours


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", NS)
def test_zero_mask_is_the_plain_outer_step(n, dtype):
    _need_gpu()
    from gym_amd import ops
    K = 8
    g = torch.Generator().manual_seed(n)
    a = _rows(K, n, n, dtype, g, False)
    b = a.clone()
    ma = torch.randn(n, generator=g).to(DEV)
    mb, va, vb = ma.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    bits = torch.zeros(ops.sparta_mask_words(n), dtype=torch.int64, device=DEV)
    for first in (True, False):
        ops.diloco_outer_masked(a, bits, ma, va, n, K, K, 0.7, 0.9, 0.0, 0.0, True, first)
        ops.diloco_outer(b, mb, vb, b, n, K, 0.7, 0.9, 0.0, 0.0, True, first)
        assert torch.equal(a, b) and torch.equal(ma, mb) and torch.equal(va, vb)
        a.add_(1.0)
        b.add_(1.0)


@pytest.mark.parametrize("K", [8, 32])
def test_the_mask_changes_the_selected_elements_only(K):
    """Non-vacuity: averaging the average is not the average.  For N(0, 1) rows
    sum_k fl(s / K) differs from s on 45% of the elements at K = 8 and 84% at
    K = 32 (and on none at K = 2 or 3), so a kernel that ignored the mask passes
    every comparison above at K <= 3 and fails this one."""
    _need_gpu()
    from gym_amd import ops
    n = N_TWO_WG
    g = torch.Generator().manual_seed(77 + K)
    a = _rows(K, n, n, torch.float32, g, False)
    b = a.clone()
    mask = _mask("random", n, g)
    ma = torch.randn(n, generator=g).to(DEV)
    mb = ma.clone()
    ops.diloco_outer_masked(a, _bits(mask), ma, None, n, K, K, 0.7, 0.0, 0.0, 0.0, False, True)
    ops.diloco_outer(b, mb, None, b, n, K, 0.7, 0.0, 0.0, 0.0, False, True)
    sel = mask.to(DEV)
    assert torch.equal(ma[~sel], mb[~sel]) and torch.equal(a[:, ~sel], b[:, ~sel])
    changed = (ma[sel] != mb[sel]).float().mean().item()
    print(f"K={K}: {changed:.3f} of the selected elements differ from the plain outer step")
    assert changed > 0
    # ...by rounding only: the K + 1 <= 33 roundings of a sum |s| < 30 (5 sigma at K = 32) move it by at most
    # 33 * 2^-24 * 30 = 6e-5; the master sees that / K * lr, plus its own last rounding (|master| < 8: 5e-7)
    torch.testing.assert_close(ma, mb, rtol=0, atol=6e-5 * 0.7 / K + 1e-6)


def test_ops_wrapper_checks():
    _need_gpu()
    from gym_amd import ops
    reps = torch.zeros(2, 128, device=DEV)
    m, bits = torch.zeros(128, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="bits"):
        ops.diloco_outer_masked(reps, bits[:1], m, None, 128, 2, 2, 0.7, 0.0, 0.0, 0.0, False, True)
    with pytest.raises(ValueError, match="bits"):
        ops.diloco_outer_masked(reps, bits.int(), m, None, 128, 2, 2, 0.7, 0.0, 0.0, 0.0, False, True)
    with pytest.raises(TypeError, match="float32"):
        ops.diloco_outer_masked(reps.bfloat16(), bits, m.bfloat16(), None, 128, 2, 2, 0.7, 0.0, 0.0, 0.0, False, True)
    with pytest.raises(ValueError, match="shorter"):
        ops.diloco_outer_masked(reps, bits, m[:64], None, 128, 2, 2, 0.7, 0.0, 0.0, 0.0, False, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.diloco_outer_masked(reps.cpu(), bits, m, None, 128, 2, 2, 0.7, 0.0, 0.0, 0.0, False, True)


# ------------------------------------------------------------ the strategy --
@pytest.fixture(scope="module")
def fused_k8():
    _need_gpu()
    return SD.run_replica_mode("sparta_diloco", 8, DEV)


def test_replica_mode_fused_equals_two_launches(fused_k8):
    _need_gpu()
    fused, s1, g1 = fused_k8
    plain, s2, g2 = SD.run_replica_mode("sparta_diloco", 8, DEV, fuse_boundary=False)
    assert s1.fuse_boundary is True and s2.fuse_boundary is False
    R.compare(plain, fused, rtol=0, atol=0)
    assert np.array_equal(g1, g2)  # the CUDA generator advanced the same way
    cfg = s1.__config__()
    assert (cfg["H"], cfg["p_sparta"], cfg["fuse_boundary"]) == (2, 0.1, True)
    assert cfg["mask_draw"] == s2.__config__()["mask_draw"] and cfg["mask_draw"] in ("fused", "torch")
    for a, b in zip(fused[0], fused[7]):  # the last step is an outer step
        assert np.array_equal(a, b)


def test_replica_mode_placement_off_is_bit_identical(fused_k8):
    _need_gpu()
    plain, s, _ = SD.run_replica_mode("sparta_diloco", 8, DEV, placement=False)
    R.compare(plain, fused_k8[0], rtol=0, atol=0)
    assert s.__config__()["placement"]["enabled"] is False
    assert s.placement_records().get("engine") == {"placed": False, "why": "placement=False"}


@pytest.mark.parametrize("name", ["sparta_diloco", "sparta_diloco_philox"])
def test_replicas_match_process_per_node_gpu(tmp_path, name):
    _need_gpu()
    proc = SD.run_process_mode(name, 3, DEV, False, str(tmp_path))["run"]
    rep, s, _ = SD.run_replica_mode(name, 3, DEV)
    assert s.fuse_boundary is (name == "sparta_diloco")
    R.compare(proc, rep)


def test_trainer_fit_four_nodes_on_one_gpu():
    _need_gpu()
    import tiny_models
    from gym_amd import LocalTrainer
    from gym_amd.strategy import SPARTADiLoCoStrategy
    from oracle.reduce import average_state_dicts
    torch.manual_seed(0)
    ds = tiny_models.dataset()
    tr = LocalTrainer(tiny_models.TinyMLP(), ds, ds, start_port=21500)
    final = tr.fit(num_epochs=1, strategy=SPARTADiLoCoStrategy(H=2, p_sparta=0.05), num_nodes=4, max_steps=6,
                   device="cuda:0", devices=[0], batch_size=32, minibatch_size=16, val_size=32, val_interval=100,
                   correlation_interval=3, keep_node_states=True)
    losses = [v for _, v in tr.run_log["train"]]
    assert len(losses) == 6 and np.isfinite(losses).all()
    nodes = [{k: v.numpy() for k, v in sd.items()} for sd in tr.node_states]
    assert len(nodes) == 4
    assert any(not np.array_equal(nodes[0][k], nodes[1][k]) for k in nodes[0])  # step 5 was an inner step
    want = average_state_dicts(nodes)
    for k, v in final.state_dict().items():
        np.testing.assert_allclose(v.numpy(), want[k], rtol=1e-6, atol=0, err_msg=k)
    got = {(step, name) for step, name, _ in tr.run_log["metrics"]}
    assert got == {(s, name) for s in (3, 6) for name in ("avg_model_correlation", "consensus_distance")}


def _forced_exchange_worker(rank, port, out_dir):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(torch.device(DEV))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        import gym_amd.strategy.strategy as strategy_mod
        from gym_amd.comm import Collective
        dev = torch.device(DEV)
        out = {}
        for tag, force in (("forced", True), ("local", False)):
            strategy_mod.Collective = lambda force=force: Collective(force_exchange=force)
            torch.manual_seed(42)
            model = R._model("x", dev)
            s = SD.make_strategy("sparta_diloco", H=1)
            s._init_node(model, 0, 2)  # a second node that never shows up: world 1
            assert s.coll.exchange is force
            out[f"{tag}_start"] = s.arena.flat.detach().cpu().numpy().copy()
            outer = s.communication_modules[1]
            communicate = outer.communicate

            def tap(model, rank, num_nodes, local_step, tag=tag, s=s, communicate=communicate):
                if local_step == 1:  # what the outer step reads: the inner step's and SPARTA's result
                    out[f"{tag}_pre"] = s.arena.flat.detach().cpu().numpy().copy()
                communicate(model, rank, num_nodes, local_step)

            outer.communicate = tap
            for t in range(2):  # H = 1: local_step 1 is the boundary step
                s.zero_grad()
                R._set_grads(model, 0, t, dev)
                s.step()
            s.finish()
            out[f"{tag}_post"] = s.arena.flat.detach().cpu().numpy().copy()
        np.savez(os.path.join(out_dir, "x.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_process_mode_boundary_step_with_a_forced_exchange(tmp_path):
    """A world-1 RCCL group with the exchange forced (as tests/test_gpu_rccl.py):
    SparseCommunicator's select / all-reduce / scatter and DiLoCoCommunicator's
    sum / all-reduce / update run one after the other on a boundary step.  With
    one rank the exchanged sums are the node's own values, so the step equals
    the local one bit for bit, and the oracle's outer step on what went in."""
    _need_gpu()
    import torch.multiprocessing as mp
    from oracle.diloco import outer_step
    from strategy_scenarios import free_port
    mp.spawn(_forced_exchange_worker, args=(free_port(), str(tmp_path)), nprocs=1, join=True)
    z = np.load(tmp_path / "x.npz")
    for k in ("start", "pre", "post"):
        assert np.array_equal(z[f"forced_{k}"], z[f"local_{k}"]), k
    assert not np.array_equal(z["forced_pre"], z["forced_start"])
    want, _, _ = outer_step(z["forced_start"], None, [z["forced_pre"]], 0.7, 0.9, True, 0.0, 0.0, 1)
    np.testing.assert_allclose(z["forced_post"], want, rtol=1e-6, atol=1e-9)  # smoke()'s bound for this kernel
    assert not np.array_equal(z["forced_post"], z["forced_pre"])
