"""Inputs and the fp32 oracle shared by the vocab-parallel cross-entropy
tests (CPU: test_vocab_parallel_ce.py, GPU: test_vocab_parallel_ce_gpu.py).

One case is a [N, 4n] bf16 logits tensor cut into w = 4 shards of width n.
The logits are randn plus a per-shard offset, so the global max lives in one
shard (+30) and another shard's term underflows in the combine (-80).
"""
import torch
import torch.nn.functional as F

W = 4
SHARD_OFFSETS = (0.0, 30.0, -80.0, 5.0)
IGNORE = -100
# (n, N): one vector with 255 idle threads; one block iteration; a second,
# partly filled block iteration; blocks looping over rows (N > grid cap 2048)
SHAPES = [(8, 37), (64, 37), (2056, 37), (64, 2051)]
# the project's CE tolerances (tests/test_ops_gpu.py::test_fused_cross_entropy)
LOSS_TOL = dict(atol=1e-2, rtol=1e-3)
GRAD_TOL = dict(atol=1e-3, rtol=5e-2)


def boundary_targets(bounds, vocab_total, N, gen, extra=()):
    """[N] int64 targets: ignore_index, the first and last column of the
    vocabulary, both columns next to every inner shard boundary (= the last
    column of one shard and the first of the next), `extra`, then random."""
    fixed = [IGNORE, 0, vocab_total - 1]
    for b in bounds[1:-1]:
        fixed += [b - 1, b]
    fixed += list(extra)
    assert len(fixed) <= N
    t = torch.randint(0, vocab_total, (N,), generator=gen)
    t[: len(fixed)] = torch.tensor(fixed)
    return t


def make_case(n, N):
    """(logits [N, 4n] bf16, target [N], dloss_rows [N] f32), on the CPU and a
    function of (n, N) alone.  Two targets are outside [0, 4n): no shard
    picks them and their gradient is scale * softmax."""
    gen = torch.Generator().manual_seed(1000 * n + N)
    V = W * n
    x = torch.randn(N, V, generator=gen)
    for s, off in enumerate(SHARD_OFFSETS):
        x[:, s * n:(s + 1) * n] += off
    bounds = [s * n for s in range(W + 1)]
    target = boundary_targets(bounds, V, N, gen, extra=(V + 5, -7))
    g_rows = torch.rand(N, generator=gen) + 0.5
    return x.bfloat16(), target, g_rows


def oracle(x32, target, reduction, g_rows=None):
    """Loss and d loss / d logits in x32's dtype.  F.cross_entropy, except
    on a row whose target is outside [0, V) and not ignore_index, which
    F.cross_entropy rejects: no class is picked, so the row's loss is its
    log-sum-exp and it counts as a non-ignored row.  The upstream gradient is
    1 for "mean" and g_rows for "none"."""
    V = x32.shape[-1]
    x = x32.detach().clone().requires_grad_(True)
    odd = (target != IGNORE) & ((target < 0) | (target >= V))
    safe = torch.where(odd, torch.zeros_like(target), target)
    rows = F.cross_entropy(x, safe, reduction="none", ignore_index=IGNORE)
    rows = torch.where(odd, torch.logsumexp(x, dim=-1), rows)
    if reduction == "none":
        rows.backward(g_rows.to(rows.dtype))
        return rows.detach(), x.grad
    loss = rows.sum() / (target != IGNORE).sum().clamp(min=1)
    loss.backward()
    return loss.detach(), x.grad


def combine(partials, target):
    """Per-row loss and global lse from per-shard (picked, lse_local), the
    way the two all-reduces combine them."""
    lse = torch.logsumexp(torch.stack([l for _, l in partials]), dim=0)
    picked = torch.stack([p for p, _ in partials]).sum(0)
    rows = torch.where(target != IGNORE, lse - picked, torch.zeros_like(lse))
    return rows, lse


def sharded_loss_and_grad(x, target, bounds, reduction, g_rows, partials_fn, grad_fn):
    """Run partials_fn / grad_fn (vp_ce_partials / vp_ce_grad signatures) on
    every shard x[:, bounds[s]:bounds[s+1]] and combine in-process."""
    V = x.shape[-1]
    shards = [x[:, a:b].contiguous() for a, b in zip(bounds[:-1], bounds[1:])]
    parts = [partials_fn(sh, target, a, V, IGNORE) for sh, a in zip(shards, bounds[:-1])]
    rows, lse = combine(parts, target)
    if reduction == "none":
        loss, drow = rows, g_rows.to(lse.dtype)
    else:
        n_tok = (target != IGNORE).sum().clamp(min=1)
        loss = rows.sum() / n_tok
        drow = torch.full_like(lse, 1.0) / n_tok
    grads = [grad_fn(sh, target, lse, drow, a, V, IGNORE) for sh, a in zip(shards, bounds[:-1])]
    return loss, torch.cat(grads, dim=-1), parts
