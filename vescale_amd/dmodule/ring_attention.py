"""Ring attention — long-context SP with O(S/p) KV memory per GPU.

SURVEY §5.7 names ring attention as the second long-context extension
("a new schedule over the p2p layer"; the reference has neither it nor
Ulysses).  Layout matches ulysses.py: q/k/v arrive [B, H, S, D] as
DTensors Shard(seq) on a 1-D mesh.  Unlike Ulysses (full-sequence KV on
every rank after the a2a), ring attention keeps only S/p keys/values
resident: the KV block circulates the ring while each rank accumulates
its query block's attention with a numerically-stable running
log-sum-exp merge — mathematically exact, not an approximation.

xGMI fit: each ring step is ONE neighbor send+recv (batched isend/irecv
pair), so the p-step ring moves each KV byte over exactly one link per
hop — the per-link-bound traffic xGMI rings are sized for — and the
next block transfers while the current one computes (the sendrecv is
posted before the block's attention math).

Autograd: the ring shift is an autograd.Function whose backward shifts
gradients the OPPOSITE way around the ring; everything else is plain
differentiable torch, so grads are exact.  Every rank executes the same
graph, so the reverse-order backward sendrecvs pair up deadlock-free.
Memory note: the default impl="eager" reference keeps per-step
O(S_local^2) score activations alive for autograd and circulates GQA keys
and values expanded to Hq heads.  impl="flash" runs every block through
ops.flash_attention (the general-shape HIP kernel on GPU, its torch
reference elsewhere), which returns (out, lse) and recomputes scores in
backward: saved state per ring step is O(S_local * D) — q, the KV block,
out and lse — and k/v travel the ring with their own Hkv heads.

Causality is exact across blocks: with q-block index i and kv-block
index j (global offsets i*S_local, j*S_local), j>i contributes nothing
(skipped — the shift still runs), j==i uses the triangular mask, j<i is
unmasked.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.distributed as dist

from ..dtensor import DTensor, Shard

__all__ = ["ring_sdpa", "RingAttention"]


class _RingShift(torch.autograd.Function):
    """out_r = in_{(r-1) % p}: send my tensor to the next rank, receive
    from the previous.  Backward shifts grads the opposite direction."""

    @staticmethod
    def forward(ctx, t: torch.Tensor, group):
        ctx.group = group
        return _shift(t, group, forward=True)

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        return _shift(g.contiguous(), ctx.group, forward=False), None


def _shift(t: torch.Tensor, group, *, forward: bool) -> torch.Tensor:
    ws = dist.get_world_size(group)
    me = dist.get_rank(group)
    nxt = dist.get_global_rank(group, (me + 1) % ws)
    prv = dist.get_global_rank(group, (me - 1) % ws)
    dst, src = (nxt, prv) if forward else (prv, nxt)
    t = t.contiguous()
    recv = torch.empty_like(t)  # empty_like of a contiguous t IS contiguous
    ops = [
        dist.P2POp(dist.isend, t, peer=dst, group=group),
        dist.P2POp(dist.irecv, recv, peer=src, group=group),
    ]
    for w in dist.batch_isend_irecv(ops):
        w.wait()
    return recv


def _merge(acc, lse, block_out, block_lse):
    """Running log-sum-exp merge of a new attention block (stable: both
    rescale factors are <= 1)."""
    new_lse = torch.logaddexp(lse, block_lse)
    acc = acc * torch.exp(lse - new_lse) + block_out * torch.exp(block_lse - new_lse)
    return acc, new_lse


def _ring_flash(ql, kl, vl, group, p, my, is_causal, scale, seg=None):
    """Ring loop over ops.flash_attention blocks.  k/v circulate with their
    own Hkv heads.  Every rank runs every block (so the shift nodes'
    backward pairs up); a future block (j > my) is passed with a shift that
    masks it wholly, and flash_attention's dead-row semantics (out = 0,
    lse = -inf, zero grads) make it a no-op in the merge.  The running
    (acc, lse) pair is fp32 and seeded from step 0 — the diagonal block,
    whose rows are all live — so the merge never sees -inf on both sides.

    seg: this rank's [B, S_local] segment ids.  The q ids stay put; the kv
    ids travel the ring next to k/v as a plain tensor (no autograd node:
    ids have no gradient) and go into every block call.  A query's own key
    carries its id, so the diagonal block's rows stay live; in a past block
    that holds nothing of a query's document the row is dead and the merge
    ignores it."""
    from ..ops import flash_attention

    s_local = ql.shape[2]
    k_cur, v_cur = kl, vl
    seg_cur = seg
    acc = lse = None
    for step in range(p):
        j = (my - step) % p  # global kv-block index currently held
        if step != p - 1:
            k_nxt = _RingShift.apply(k_cur, group)
            v_nxt = _RingShift.apply(v_cur, group)
            if seg is not None:
                seg_nxt = _shift(seg_cur, group, forward=True)
        masked = is_causal and j >= my  # past blocks (j < my) are fully visible
        block_out, block_lse = flash_attention(
            ql, k_cur, v_cur,
            is_causal=masked,
            causal_shift=(my - j) * s_local if masked else 0,
            scale=scale, return_lse=True,
            q_segment_ids=seg, kv_segment_ids=seg_cur,
        )
        block_out = block_out.float()
        block_lse = block_lse.float().unsqueeze(-1)
        if step == 0:
            acc, lse = block_out, block_lse
        else:
            acc, lse = _merge(acc, lse, block_out, block_lse)
        if step != p - 1:
            k_cur, v_cur = k_nxt, v_nxt
            if seg is not None:
                seg_cur = seg_nxt
    return acc.to(ql.dtype)


def ring_sdpa(
    q: DTensor,
    k: DTensor,
    v: DTensor,
    *,
    is_causal: bool = False,
    scale: Optional[float] = None,
    seq_dim: int = 2,
    impl: str = "eager",
    segment_ids: Optional[torch.Tensor] = None,
) -> DTensor:
    """Exact sequence-parallel attention with ring-circulated KV.

    q/k/v: DTensors [B, H, S, D] Shard(seq_dim) on a 1-D mesh; returns
    the same layout.  GQA (fewer KV heads) works: KV heads broadcast over
    the query-head grouping like F.scaled_dot_product_attention with
    enable_gqa.  impl="flash" computes each block with ops.flash_attention
    (see the module docstring's memory note); it needs the default
    [B, H, S, D] layout (seq_dim == 2).

    segment_ids: this rank's local [B, S_local] slice (a plain integer
    tensor) of the packed rows' [B, S] segment ids; a token attends only to
    tokens with its own id, across ranks too.  impl="flash" only.
    """
    assert impl in ("eager", "flash"), f"unknown impl {impl!r}"
    if segment_ids is not None and impl != "flash":
        raise ValueError("ring_sdpa: segment_ids needs impl='flash'")
    mesh = q.device_mesh
    assert mesh.ndim == 1, "ring_sdpa runs over a 1-D (SP) mesh"
    for name, t in (("q", q), ("k", k), ("v", v)):
        assert isinstance(t, DTensor) and t.placements[0].is_shard(seq_dim), (
            f"{name} must be Shard({seq_dim})"
        )
    group = mesh.get_group(0)
    p = dist.get_world_size(group)
    my = dist.get_rank(group)

    ql, kl, vl = q.to_local(), k.to_local(), v.to_local()
    B, Hq, Sq, D = ql.shape
    Hk = kl.shape[1]
    assert Hq % Hk == 0, "query heads must be a multiple of kv heads (GQA)"
    if impl == "flash":
        assert seq_dim == 2, "impl='flash' needs the [B, H, S, D] layout"
        seg = None
        if segment_ids is not None:
            if tuple(segment_ids.shape) != (B, Sq):
                raise ValueError(
                    f"ring_sdpa: segment_ids must be the local [B, S_local] = "
                    f"[{B}, {Sq}] slice, got {list(segment_ids.shape)}")
            seg = segment_ids.to(torch.int32).contiguous()
        out = _ring_flash(ql, kl, vl, group, p, my, is_causal, scale, seg)
        return DTensor.from_local(out, mesh, [Shard(seq_dim)])
    if Hk != Hq:
        rep = Hq // Hk
        kl = kl.repeat_interleave(rep, dim=1)
        vl = vl.repeat_interleave(rep, dim=1)
    sc = scale if scale is not None else 1.0 / math.sqrt(D)

    acc = torch.zeros_like(ql)
    lse = torch.full((B, Hq, Sq, 1), float("-inf"), dtype=ql.dtype, device=ql.device)
    # FINITE mask value, not -inf: every rank must compute EVERY block so
    # the autograd graph (incl. the ring-shift nodes) is identical across
    # ranks — a rank that skipped its last block would never run that
    # shift's backward and deadlock the ring.  exp(neg) underflows to 0,
    # so fully-masked blocks contribute nothing but still carry (zero)
    # gradient through k_cur/v_cur.
    neg = torch.finfo(ql.dtype).min / 2
    causal_mask = None
    if is_causal:
        causal_mask = torch.triu(
            torch.full((Sq, kl.shape[2]), neg, device=ql.device, dtype=ql.dtype),
            diagonal=1,
        )

    k_cur, v_cur = kl, vl
    for step in range(p):
        j = (my - step) % p  # global kv-block index currently held
        # post the next shift before the block math (on GPU the sendrecv
        # runs on the comm stream while the block computes)
        if step != p - 1:
            k_nxt = _RingShift.apply(k_cur, group)
            v_nxt = _RingShift.apply(v_cur, group)
        scores = (ql @ k_cur.transpose(-1, -2)) * sc
        if is_causal:
            if j == my:
                scores = scores + causal_mask
            elif j > my:
                scores = scores + neg  # future block: no contribution
        block_lse = scores.logsumexp(-1, keepdim=True)
        block_out = torch.softmax(scores, dim=-1) @ v_cur
        acc, lse = _merge(acc, lse, block_out, block_lse)
        if step != p - 1:
            k_cur, v_cur = k_nxt, v_nxt

    return DTensor.from_local(acc, mesh, [Shard(seq_dim)])


class RingAttention(torch.nn.Module):
    """Module wrapper mirroring UlyssesAttention."""

    def __init__(self, *, is_causal: bool = False, scale: Optional[float] = None,
                 impl: str = "eager"):
        super().__init__()
        self.is_causal = is_causal
        self.scale = scale
        self.impl = impl

    def forward(self, q: DTensor, k: DTensor, v: DTensor,
                segment_ids: Optional[torch.Tensor] = None) -> DTensor:
        return ring_sdpa(q, k, v, is_causal=self.is_causal, scale=self.scale,
                         impl=self.impl, segment_ids=segment_ids)
