"""Vocab-parallel cross-entropy kernels (ce_vp_fwd_bf16 / ce_vp_bwd_bf16 in
ops/csrc/cross_entropy.hip) on the GPU: w = 4 shards cut from one [N, 4n]
bf16 tensor and handed to the kernels as contiguous slices of a NaN-filled
arena, combined in-process the way the two all-reduces combine them.

lse_local accuracy bound, truth = torch.logsumexp of the shard in fp64 and
the yardstick the dense ce_fwd kernel on the same shard:

    max_err_new <= 4 * max_err_dense + 2^-22 * max|lse|

The factor 4 covers a different summation order and a different number of
exponentials per element, the additive term one fp32 rounding of the result.
Several ranks on several GPUs are not run here (single-GPU machines): the
gloo tests of test_vocab_parallel_ce.py cover the collective wiring.
"""
import dataclasses
import functools

import pytest
import torch

from tests.vp_ce_cases import (
    GRAD_TOL, IGNORE, LOSS_TOL, SHAPES, W, make_case, oracle, sharded_loss_and_grad,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

PAD = 4096  # NaN elements on each side of every arena slice
NAN_BITS = torch.tensor(float("nan"), dtype=torch.bfloat16).view(torch.int16).item()


def _arena_shards(x):
    """The W column shards of x [N, W*n] as contiguous [N, n] slices of one
    all-NaN bf16 arena, with the arena and its outside-the-slices mask."""
    N, n = x.shape[0], x.shape[1] // W
    total = PAD + W * (N * n + PAD)
    arena = torch.full((total,), float("nan"), device="cuda", dtype=torch.bfloat16)
    outside = torch.ones(total, dtype=torch.bool, device="cuda")
    shards, off = [], PAD
    for s in range(W):
        arena[off:off + N * n] = x[:, s * n:(s + 1) * n].reshape(-1)
        outside[off:off + N * n] = False
        shards.append(arena[off:off + N * n].view(N, n))
        off += N * n + PAD
    return shards, arena, outside


@functools.lru_cache(maxsize=None)
def _results(n, N):
    import vescale_amd.ops as ops

    C = ops.require_ext()
    x_cpu, t_cpu, g_cpu = make_case(n, N)
    x, target, g_rows = x_cpu.cuda(), t_cpu.cuda(), g_cpu.cuda()
    V = W * n
    shards, arena, outside = _arena_shards(x)
    fwd = [C.ce_fwd(sh, target, IGNORE, vocab_start=s * n, vocab_total=V)
           for s, sh in enumerate(shards)]
    fwd2 = [C.ce_fwd(sh, target, IGNORE, vocab_start=s * n, vocab_total=V)
            for s, sh in enumerate(shards)]
    dense = [C.ce_fwd(sh, target.clamp(0, n - 1), IGNORE) for sh in shards]
    truth = [torch.logsumexp(sh.double(), dim=-1) for sh in shards]
    # the ops wrappers on the arena slices: loss and concatenated gradients
    out = {}
    for reduction in ("mean", "none"):
        out[reduction] = sharded_loss_and_grad(
            x, target, [s * n for s in range(W + 1)], reduction, g_rows,
            lambda sh, t, a, v, ig: ops.vp_ce_partials(shards[a // n], t, a, v, ig),
            lambda sh, t, l, d, a, v, ig: ops.vp_ce_grad(shards[a // n], t, l, d, a, v, ig))[:2]
    torch.cuda.synchronize()
    arena_ok = bool((arena.view(torch.int16)[outside] == NAN_BITS).all())
    ref = {r: oracle(x.float(), target, r, g_rows) for r in ("mean", "none")}
    return dict(x=x, target=target, g_rows=g_rows, shards=shards, arena=arena,
                outside=outside, fwd=fwd, fwd2=fwd2, dense=dense, truth=truth,
                out=out, ref=ref, arena_ok=arena_ok)


@requires_gpu
@pytest.mark.parametrize("n,N", SHAPES)
def test_picked_is_the_raw_target_logit_or_zero(n, N):
    r = _results(n, N)
    x, target = r["x"], r["target"]
    assert r["arena_ok"]
    assert ((target == W * n + 5) | (target == -7)).sum() == 2
    for s, (picked, _) in enumerate(r["fwd"]):
        hit = (target != IGNORE) & (target >= s * n) & (target < (s + 1) * n)
        raw = x.float().gather(1, target.clamp(0, W * n - 1)[:, None])[:, 0]
        want = torch.where(hit, raw, torch.zeros_like(raw))
        assert picked.dtype == torch.float32
        assert torch.equal(picked.view(torch.int32), want.view(torch.int32)), (n, N, s)


@requires_gpu
@pytest.mark.parametrize("n,N", SHAPES)
def test_lse_local_accuracy_against_dense_kernel(n, N):
    r = _results(n, N)
    for s in range(W):
        truth = r["truth"][s]
        err_new = (r["fwd"][s][1].double() - truth).abs().max().item()
        err_dense = (r["dense"][s][1].double() - truth).abs().max().item()
        tol = 4 * err_dense + 2.0 ** -22 * truth.abs().max().item()
        print(f"lse_local n={n} N={N} shard={s}: err_new {err_new:.3e} "
              f"err_dense {err_dense:.3e} tol {tol:.3e}")
        assert err_new <= tol, (n, N, s, err_new, err_dense, tol)


@requires_gpu
@pytest.mark.parametrize("reduction", ["mean", "none"])
@pytest.mark.parametrize("n,N", SHAPES)
def test_end_to_end_against_fp32_cross_entropy(n, N, reduction):
    r = _results(n, N)
    loss, grad = r["out"][reduction]
    ref_loss, ref_grad = r["ref"][reduction]
    assert r["arena_ok"]
    assert grad.dtype == torch.bfloat16 and grad.shape == r["x"].shape
    print(f"e2e n={n} N={N} {reduction}: loss err {(loss - ref_loss).abs().max().item():.3e} "
          f"grad err {(grad.float() - ref_grad).abs().max().item():.3e}")
    assert torch.allclose(loss, ref_loss, **LOSS_TOL)
    assert torch.allclose(grad.float(), ref_grad, **GRAD_TOL)
    # out-of-vocabulary targets: scale * softmax, nothing subtracted
    odd = (r["target"] == W * n + 5) | (r["target"] == -7)
    assert (grad.float()[odd] >= 0).all()


@requires_gpu
@pytest.mark.parametrize("n,N", SHAPES)
def test_inplace_backward_and_repeatability(n, N):
    import vescale_amd.ops as ops

    C = ops.require_ext()
    r = _results(n, N)
    target, V = r["target"], W * n
    for (pa, la), (pb, lb) in zip(r["fwd"], r["fwd2"]):
        assert torch.equal(pa.view(torch.int32), pb.view(torch.int32))
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    lse = torch.logsumexp(torch.stack([l for _, l in r["fwd"]]), dim=0)
    for s, sh in enumerate(r["shards"]):
        args = (target, lse, r["g_rows"], IGNORE)
        a = C.ce_bwd(sh, *args, False, vocab_start=s * n, vocab_total=V)
        b = C.ce_bwd(sh, *args, False, vocab_start=s * n, vocab_total=V)
        assert a.data_ptr() != sh.data_ptr()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        saved = sh.clone()
        c = C.ce_bwd(sh, *args, True, vocab_start=s * n, vocab_total=V)
        assert c.data_ptr() == sh.data_ptr() and c.shape == sh.shape
        assert torch.equal(c.view(torch.int16), a.view(torch.int16))
        assert torch.equal(sh.view(torch.int16), a.view(torch.int16))
        sh.copy_(saved)  # the cached case keeps its inputs
    torch.cuda.synchronize()
    arena = r["arena"]
    assert bool((arena.view(torch.int16)[r["outside"]] == NAN_BITS).all())


@requires_gpu
@pytest.mark.parametrize("n,N", [(64, 37), (2056, 37)])
def test_one_shard_agrees_with_fused_cross_entropy(n, N):
    from vescale_amd.ops import fused_cross_entropy, vocab_parallel_cross_entropy

    x_cpu, t_cpu, _ = make_case(n, N)
    V = W * n
    target = torch.where((t_cpu < 0) | (t_cpu >= V), torch.full_like(t_cpu, IGNORE), t_cpu).cuda()
    a = x_cpu.cuda().requires_grad_(True)
    b = x_cpu.cuda().requires_grad_(True)
    la = vocab_parallel_cross_entropy(a, target, 0, V, group=None, ignore_index=IGNORE)
    lb = fused_cross_entropy(b, target, IGNORE)
    la.backward()
    lb.backward()
    assert torch.allclose(la, lb, **LOSS_TOL), (la, lb)
    assert torch.allclose(a.grad.float(), b.grad.float(), **GRAD_TOL)


@requires_gpu
def test_world1_vocab_parallel_head_is_a_no_op():
    from vescale_amd.models.llama import LlamaModel, llama_tiny
    from vescale_amd.models.llama_tp import TPContext

    cfg = llama_tiny()
    torch.manual_seed(3)
    a = LlamaModel(cfg)
    a.init_weights()
    # the issue's "world-1 TP context": no group, so TPContext.single()
    b = LlamaModel(dataclasses.replace(cfg, vocab_parallel_head=True), tp_group=None)
    b.load_state_dict(a.state_dict())
    a, b = a.cuda().to(torch.bfloat16), b.cuda().to(torch.bfloat16)
    for m in (a, b):
        m.rope_table.data = m.rope_table.data.float()
    assert b.tp == TPContext.single() and not b.vp_head
    x = torch.randint(0, cfg.vocab_size, (2, 64), device="cuda")
    y = torch.roll(x, -1, dims=1)
    la, lb = a(x, y), b(x, y)
    la.backward()
    lb.backward()
    assert la.isfinite() and torch.equal(la, lb)
    for (na, pa), (nb, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert na == nb and torch.equal(pa.grad, pb.grad), na
