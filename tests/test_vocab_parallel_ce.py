"""Vocab-parallel cross-entropy on the CPU: the torch path of the building
blocks against F.cross_entropy (in-process shards), the collective wiring
of ops.vocab_parallel_cross_entropy over gloo, and the Llama vocab-parallel
head against the replicated-head model."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from tests.common import spawn
from tests.vp_ce_cases import (
    GRAD_TOL, IGNORE, LOSS_TOL, SHAPES, W, boundary_targets, make_case, oracle,
    sharded_loss_and_grad,
)

from vescale_amd.ops import (
    fused_cross_entropy, vocab_parallel_cross_entropy, vp_ce_grad, vp_ce_partials,
)

@pytest.fixture(autouse=True)
def _no_intra_op_pool():
    """The in-process math here must not start the intra-op thread pool:
    the spawn tests of this and of later files fork this process, and a
    forked child of a process with a live OpenMP pool hangs in its first
    parallel region."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


N, V = 9, 40
# even; uneven; uneven with a shard of width 1 at the start, inside, at the end
SPLITS = {
    "even4": [0, 10, 20, 30, 40],
    "uneven": [0, 7, 30, 40],
    "width1_first": [0, 1, 24, 40],
    "width1_inner": [0, 13, 14, 40],
    "width1_last": [0, 16, 39, 40],
    "one_shard": [0, 40],
}


def _inputs(bounds):
    gen = torch.Generator().manual_seed(11 + len(bounds))
    x = torch.randn(N, V, generator=gen)
    target = boundary_targets(bounds, V, N, gen)
    g_rows = torch.rand(N, generator=gen) + 0.5
    return x, target, g_rows


@pytest.mark.parametrize("reduction", ["mean", "none"])
@pytest.mark.parametrize("split", sorted(SPLITS))
def test_in_process_shards_match_dense(split, reduction):
    bounds = SPLITS[split]
    x, target, g_rows = _inputs(bounds)
    assert (target == IGNORE).any()
    loss, grad, parts = sharded_loss_and_grad(
        x, target, bounds, reduction, g_rows, vp_ce_partials, vp_ce_grad)
    # the oracle here is F.cross_entropy itself: every target is a class
    xr = x.clone().requires_grad_(True)
    ref = F.cross_entropy(xr, target, ignore_index=IGNORE, reduction=reduction)
    ref.backward(g_rows if reduction == "none" else None)
    assert torch.allclose(loss, ref.detach(), atol=1e-5), (loss, ref)
    assert torch.allclose(grad, xr.grad, atol=1e-5), (grad - xr.grad).abs().max()
    # picked: the raw target logit on exactly one shard, exactly 0 elsewhere
    for (picked, _), a, b in zip(parts, bounds[:-1], bounds[1:]):
        hit = (target != IGNORE) & (target >= a) & (target < b)
        want = torch.where(hit, x.gather(1, target.clamp(min=0)[:, None])[:, 0],
                           torch.zeros(N))
        assert torch.equal(picked, want)


@pytest.mark.parametrize("split", ["even4", "width1_inner"])
def test_all_ignored_batch(split):
    bounds = SPLITS[split]
    x, _, g_rows = _inputs(bounds)
    target = torch.full((N,), IGNORE)
    for reduction in ("mean", "none"):
        loss, grad, _ = sharded_loss_and_grad(
            x, target, bounds, reduction, g_rows, vp_ce_partials, vp_ce_grad)
        assert torch.equal(loss, torch.zeros_like(loss))
        assert torch.equal(grad, torch.zeros_like(grad))


def test_out_of_vocabulary_targets_pick_nothing():
    x, target, _ = _inputs(SPLITS["even4"])
    target[1], target[2] = V + 5, -7
    for a, b in zip(SPLITS["even4"][:-1], SPLITS["even4"][1:]):
        picked, _ = vp_ce_partials(x[:, a:b], target, a, V, IGNORE)
        assert picked[1] == 0 and picked[2] == 0


def test_single_shard_is_fused_cross_entropy():
    x, target, _ = _inputs(SPLITS["one_shard"])
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    la = vocab_parallel_cross_entropy(a, target, 0, V, group=None, ignore_index=IGNORE)
    lb = fused_cross_entropy(b, target, IGNORE)
    la.backward()
    lb.backward()
    assert torch.allclose(la, lb, atol=1e-6)
    assert torch.allclose(a.grad, b.grad, atol=1e-6)


def test_bad_shard_range_is_refused():
    x, target, _ = _inputs(SPLITS["even4"])
    with pytest.raises(ValueError, match="not inside"):
        vp_ce_partials(x[:, :10], target, 35, V, IGNORE)
    with pytest.raises(ValueError, match="not inside"):
        vp_ce_partials(x[:, :10], target, -1, V, IGNORE)
    with pytest.raises(ValueError, match="reduction"):
        vocab_parallel_cross_entropy(x, target, 0, V, reduction="sum")


@pytest.mark.parametrize("n,rows", SHAPES)
def test_reference_meets_project_tolerances_on_gpu_inputs(n, rows):
    """The GPU tests hold the kernels to the project's CE tolerances against
    the fp32 oracle on these inputs; the torch path on the bf16-rounded
    inputs (bf16 gradients out) must itself be inside them."""
    x, target, g_rows = make_case(n, rows)
    bounds = [s * n for s in range(W + 1)]
    for reduction in ("mean", "none"):
        loss, grad, _ = sharded_loss_and_grad(
            x, target, bounds, reduction, g_rows, vp_ce_partials, vp_ce_grad)
        ref_loss, ref_grad = oracle(x.float(), target, reduction, g_rows)
        assert grad.dtype == torch.bfloat16
        assert torch.allclose(loss, ref_loss, **LOSS_TOL)
        assert torch.allclose(grad.float(), ref_grad, **GRAD_TOL)


# --------------------------- two ranks over gloo ---------------------------
def _t_collectives(rank, ws):
    import torch.distributed as dist

    gen = torch.Generator().manual_seed(23)
    rows, vocab = 7, 24
    x = torch.randn(rows, vocab, generator=gen)
    x[:, vocab // 2:] += 20.0  # the max lives on rank 1
    target = boundary_targets([0, vocab // 2, vocab], vocab, rows, gen)
    g_rows = torch.rand(rows, generator=gen) + 0.5
    n = vocab // ws
    calls = []
    orig = dist.all_reduce

    def counting(tensor, *a, **k):
        calls.append((tensor.dtype, tensor.numel()))
        return orig(tensor, *a, **k)

    for reduction in ("mean", "none"):
        ref_loss, ref_grad = oracle(x, target, reduction, g_rows)
        local = x[:, rank * n:(rank + 1) * n].clone().requires_grad_(True)
        dist.all_reduce = counting
        try:
            calls.clear()
            loss = vocab_parallel_cross_entropy(
                local, target, rank * n, vocab, group=dist.group.WORLD,
                ignore_index=IGNORE, reduction=reduction)
            fwd = list(calls)
            calls.clear()
            loss.backward(g_rows if reduction == "none" else None)
            bwd = list(calls)
        finally:
            dist.all_reduce = orig
        assert len(fwd) <= 2, fwd
        assert sorted(fwd) == [(torch.float32, rows), (torch.float32, 2 * rows)], fwd
        assert bwd == [], bwd
        assert torch.allclose(loss, ref_loss, atol=1e-5), (loss, ref_loss)
        want = ref_grad[:, rank * n:(rank + 1) * n]
        assert torch.allclose(local.grad, want, atol=1e-5), (local.grad - want).abs().max()


def test_two_ranks_two_collectives():
    spawn(2, _t_collectives)


def _t_vp_head_parity(rank, ws):
    """test_llama_tp2_parity with the vocab-parallel head, and its tolerances."""
    import torch.distributed as dist

    from vescale_amd.models.llama import LlamaModel, llama_tiny
    from vescale_amd.models.llama_tp import shard_llama_state_dict

    torch.manual_seed(5)
    cfg = llama_tiny()
    ref = LlamaModel(cfg)
    ref.init_weights()
    x = torch.randint(0, cfg.vocab_size, (2, 32))
    y = torch.roll(x, -1, dims=1)
    y[0, :3] = -100
    ref_loss = ref(x, y)
    ref_loss.backward()

    cfg_vp = dataclasses.replace(cfg, vocab_parallel_head=True)
    tp_model = LlamaModel(cfg_vp, tp_group=dist.group.WORLD)
    assert tp_model.output.weight.shape == (cfg.vocab_size // ws, cfg.dim)
    full_sd = {k: v.detach() for k, v in ref.state_dict().items()}
    tp_model.load_state_dict(
        shard_llama_state_dict(full_sd, cfg, rank, ws, vocab_parallel_head=True))
    loss = tp_model(x, y)
    assert torch.allclose(loss, ref_loss.detach(), atol=2e-5), (float(loss), float(ref_loss))
    loss.backward()
    gs = shard_llama_state_dict(
        {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in ref.named_parameters()},
        cfg, rank, ws, vocab_parallel_head=True,
    )
    seen = set()
    for name, p in tp_model.named_parameters():
        assert p.grad is not None, name
        want = gs[name]
        assert p.grad.shape == want.shape, name
        assert torch.allclose(p.grad, want, atol=5e-5), (name, (p.grad - want).abs().max())
        seen.add(name)
    assert "output.weight" in seen
    # no targets: callers still see [B, S, V] logits
    with torch.no_grad():
        logits = tp_model(x)
        ref_logits = ref(x)
    assert logits.shape == ref_logits.shape == (2, 32, cfg.vocab_size)
    assert torch.allclose(logits, ref_logits, atol=2e-5), (logits - ref_logits).abs().max()


def test_llama_tp2_vocab_parallel_head_parity():
    spawn(2, _t_vp_head_parity)


def test_vocab_parallel_head_is_a_no_op_without_tp():
    from vescale_amd.models.llama import LlamaModel, llama_tiny

    cfg = llama_tiny()
    torch.manual_seed(3)
    a = LlamaModel(cfg)
    a.init_weights()
    b = LlamaModel(dataclasses.replace(cfg, vocab_parallel_head=True))
    b.load_state_dict(a.state_dict())
    x = torch.randint(0, cfg.vocab_size, (2, 16))
    y = torch.roll(x, -1, dims=1)
    assert torch.equal(a(x, y), b(x, y))
