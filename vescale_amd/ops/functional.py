"""Autograd wrappers for the CDNA4 HIP kernels, with pure-torch reference
implementations used (a) on CPU boxes for tests, (b) as the fp32 numerics
oracle the GPU tests compare against (SURVEY.md §4 test strategy)."""
from __future__ import annotations

from typing import Optional

import os

import torch


def _ext():
    """The extension module.  Its bindings validate and never copy: every
    tensor handed to them below is made contiguous first."""
    from . import require_ext

    return require_ext()


def _use_hip(*tensors) -> bool:
    from . import has_ext

    on_gpu = all(t.is_cuda for t in tensors if isinstance(t, torch.Tensor))
    if not on_gpu:
        return False
    if not has_ext():
        # loud failure: GPU present but no extension
        from . import require_ext

        require_ext()
    return True


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------
class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, eps: float):
        if _use_hip(x, weight):
            x2, w2 = x.contiguous(), weight.contiguous()
            out, rrms = _ext().rmsnorm_fwd(x2, w2, eps)
            ctx.save_for_backward(x2, w2, rrms)
            ctx.eps = eps
            ctx.hip = True
            return out
        # reference (fp32 math)
        xf = x.float()
        rrms = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        out = (xf * rrms * weight.float()).to(x.dtype)
        ctx.save_for_backward(x, weight, rrms.squeeze(-1))
        ctx.eps = eps
        ctx.hip = False
        return out

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w, rrms = ctx.saved_tensors
        if ctx.hip:
            dx, dw = _ext().rmsnorm_bwd(dy.contiguous(), x, w, rrms)
            return dx, dw.to(w.dtype), None
        xf = x.float()
        dyf = dy.float()
        wf = w.float()
        r = rrms.unsqueeze(-1)
        H = x.shape[-1]
        dot = (dyf * wf * xf).sum(-1, keepdim=True)
        dx = (r * wf * dyf - xf * dot * r.pow(3) / H).to(x.dtype)
        dw = (dyf * xf * r).reshape(-1, H).sum(0).to(w.dtype)
        return dx, dw, None


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    return _RMSNorm.apply(x, weight, eps)


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------
def build_rope_table(
    seq_len: int, head_dim: int, theta: float = 500000.0, device="cpu"
) -> torch.Tensor:
    """[S, D/2, 2] fp32 (cos, sin) — host-precomputed (guide App. B: no
    on-device trig)."""
    rot = head_dim // 2
    # explicit cpu device so meta-device init contexts don't capture these
    inv = 1.0 / (theta ** (torch.arange(0, rot, dtype=torch.float64, device="cpu") / rot))
    pos = torch.arange(seq_len, dtype=torch.float64, device="cpu")
    ang = torch.outer(pos, inv)
    tab = torch.stack([ang.cos(), ang.sin()], dim=-1).to(torch.float32)
    return tab.to(device)


class _RoPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, table: torch.Tensor, pos_offset: int):
        ctx.pos_offset = pos_offset
        if _use_hip(x, table):
            ctx.hip = True
            ctx.save_for_backward(table)
            return _ext().rope(x.contiguous(), table.contiguous(), pos_offset, False, False)
        ctx.hip = False
        ctx.save_for_backward(table)
        return _rope_ref(x, table, pos_offset, False)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        (table,) = ctx.saved_tensors
        if ctx.hip:
            return _ext().rope(dy.contiguous(), table.contiguous(), ctx.pos_offset, True, False), None, None
        return _rope_ref(dy, table, ctx.pos_offset, True), None, None


def _rope_ref(x, table, pos_offset, backward):
    B, S, H, D = x.shape
    rot = D // 2
    tb = table[pos_offset : pos_offset + S]  # [S, rot, 2]
    cos = tb[..., 0].unsqueeze(0).unsqueeze(2)  # [1,S,1,rot]
    sin = tb[..., 1].unsqueeze(0).unsqueeze(2)
    if backward:
        sin = -sin
    xf = x.float()
    x0, x1 = xf[..., :rot], xf[..., rot:]
    o0 = x0 * cos - x1 * sin
    o1 = x1 * cos + x0 * sin
    return torch.cat([o0, o1], dim=-1).to(x.dtype)


class _FusedAddRMSNorm(torch.autograd.Function):
    """Residual-stream add fused into RMSNorm: (x, res) -> (norm(x+res),
    x+res).  res may be None (start of the stream).  Backward fuses the
    residual grad accumulation into the norm backward (kernel dres path).
    The grad w.r.t. x and res is the same tensor (add distributes)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, res, weight: torch.Tensor, eps: float):
        ctx.has_res = res is not None
        if _use_hip(x, weight) and (res is None or res.dtype == x.dtype):
            w2 = weight.contiguous()
            out, res_new, rrms = _ext().rmsnorm_res_fwd(
                x.contiguous(), res.contiguous() if res is not None else None,
                w2, eps,
            )
            ctx.save_for_backward(res_new, w2, rrms)
            ctx.hip = True
            return out, res_new
        res_new = x if res is None else (x + res)
        xf = res_new.float()
        rrms = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        out = (xf * rrms * weight.float()).to(x.dtype)
        ctx.save_for_backward(res_new, weight, rrms.squeeze(-1))
        ctx.hip = False
        return out, res_new

    @staticmethod
    def backward(ctx, dy: torch.Tensor, dres_new):
        res_new, w, rrms = ctx.saved_tensors
        if ctx.hip:
            dx, dw = _ext().rmsnorm_bwd(
                dy.contiguous(), res_new, w, rrms,
                dres_new.contiguous() if dres_new is not None else None,
            )
            dw = dw.to(w.dtype)
        else:
            xf = res_new.float()
            dyf = dy.float()
            r = rrms.unsqueeze(-1)
            wf = w.float()
            h = res_new.shape[-1]
            dot = (dyf * wf * xf).sum(-1, keepdim=True)
            dx = (r * wf * dyf - xf * (dot * r.pow(3) / h)).to(res_new.dtype)
            dw = (dyf * xf * r).reshape(-1, h).sum(0).to(w.dtype)
            if dres_new is not None:
                dx = dx + dres_new
        dres = dx if ctx.has_res else None
        return dx, dres, dw, None


def fused_add_rmsnorm(x, res, weight, eps):
    """(norm(x + res), x + res); res=None starts the residual stream."""
    return _FusedAddRMSNorm.apply(x, res, weight, eps)


def rope_apply(x: torch.Tensor, table: torch.Tensor, pos_offset: int = 0) -> torch.Tensor:
    """x: [B, S, H, D]."""
    return _RoPE.apply(x, table, pos_offset)


class _RoPEQKV(torch.autograd.Function):
    """Fused qkv-split + RoPE (packed wqkv GEMM output -> q/k/v)."""

    @staticmethod
    def forward(ctx, qkv: torch.Tensor, table: torch.Tensor, n_heads: int,
                n_kv_heads: int, head_dim: int, pos_offset: int):
        B, S, _ = qkv.shape
        ctx.dims = (B, S, n_heads, n_kv_heads, head_dim, pos_offset)
        ctx.save_for_backward(table)
        if _use_hip(qkv, table):
            ctx.hip = True
            q, k, v = _ext().rope_qkv_fwd(
                qkv.contiguous(), table.contiguous(), B, S, n_heads, n_kv_heads, head_dim,
                pos_offset,
            )
            return q, k, v
        ctx.hip = False
        d = n_heads * head_dim
        kv = n_kv_heads * head_dim
        q = qkv[..., :d].reshape(B, S, n_heads, head_dim)
        k = qkv[..., d : d + kv].reshape(B, S, n_kv_heads, head_dim)
        v = qkv[..., d + kv :].reshape(B, S, n_kv_heads, head_dim)
        q = _rope_ref(q, table, pos_offset, False)
        k = _rope_ref(k, table, pos_offset, False)
        # match the HIP kernel's [B, H, S, D] output layout
        return (
            q.permute(0, 2, 1, 3).contiguous(),
            k.permute(0, 2, 1, 3).contiguous(),
            v.permute(0, 2, 1, 3).contiguous(),
        )

    @staticmethod
    def backward(ctx, dq, dk, dv):
        (table,) = ctx.saved_tensors
        B, S, Hq, Hkv, D, pos = ctx.dims
        if ctx.hip:
            dqkv = _ext().rope_qkv_bwd(
                dq.contiguous(), dk.contiguous(), dv.contiguous(),
                table.contiguous(), B, S, Hq, Hkv, D, pos,
            )
            return dqkv, None, None, None, None, None
        dq = dq.permute(0, 2, 1, 3)  # [B,H,S,D] -> [B,S,H,D]
        dk = dk.permute(0, 2, 1, 3)
        dv = dv.permute(0, 2, 1, 3)
        dqr = _rope_ref(dq, table, pos, True).reshape(B, S, Hq * D)
        dkr = _rope_ref(dk, table, pos, True).reshape(B, S, Hkv * D)
        dvr = dv.reshape(B, S, Hkv * D)
        return torch.cat([dqr, dkr, dvr], dim=-1), None, None, None, None, None


def rope_qkv(qkv: torch.Tensor, table: torch.Tensor, n_heads: int,
             n_kv_heads: int, head_dim: int, pos_offset: int = 0):
    """qkv: [B, S, (Hq+2*Hkv)*D] packed -> (q, k, v) in [B, H, S, D] (the
    attention kernels' native layout), RoPE applied to q and k."""
    return _RoPEQKV.apply(qkv, table, n_heads, n_kv_heads, head_dim, pos_offset)


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------
def _swiglu_dup(d, g, sig):
    """dy * silu(gate) as the kernels take it (swiglu_dup in swiglu.hip):
    (dy * gate) * sig, or dy * (gate * sig) where dy * gate overflows."""
    t = d * g
    return torch.where(t.isinf(), d * (g * sig), t * sig)


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate: torch.Tensor, up: torch.Tensor):
        if _use_hip(gate, up):
            g = gate.contiguous()
            u = up.contiguous()
            ctx.save_for_backward(g, u)
            ctx.hip = True
            return _ext().swiglu_fwd(g, u)
        ctx.save_for_backward(gate, up)
        ctx.hip = False
        return (torch.nn.functional.silu(gate.float()) * up.float()).to(gate.dtype)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        gate, up = ctx.saved_tensors
        if ctx.hip:
            dgate, dup = _ext().swiglu_bwd(dy.contiguous(), gate, up)
            return dgate, dup
        g = gate.float()
        u = up.float()
        d = dy.float()
        sig = torch.sigmoid(g)
        dgate = (d * u * sig * (1 + g * (1 - sig))).to(gate.dtype)
        dup = _swiglu_dup(d, g, sig).to(up.dtype)
        return dgate, dup


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    return _SwiGLU.apply(gate, up)


class _SwiGLUPacked(torch.autograd.Function):
    """gu = [.., 2F] (gate||up) -> [.., F]; avoids split+cat round trips.

    want_t: the producer of gu is a dense linear whose wgrad takes dgu^T
    (linear() marks its output, see _WGRAD_T).  The backward then asks the
    kernel for dgu^T as a second output of the same pass and hands it over
    as an attribute of dgu; _LinearWgrad.backward takes it off again."""

    @staticmethod
    def forward(ctx, gu: torch.Tensor, want_t: bool = False):
        if _use_hip(gu):
            g = gu.contiguous()
            ctx.save_for_backward(g)
            ctx.hip = True
            ctx.want_t = want_t
            return _ext().swiglu_packed_fwd(g)
        ctx.save_for_backward(gu)
        ctx.hip = False
        F = gu.shape[-1] // 2
        gate, up = gu[..., :F], gu[..., F:]
        return (torch.nn.functional.silu(gate.float()) * up.float()).to(gu.dtype)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        (gu,) = ctx.saved_tensors
        if ctx.hip:
            if ctx.want_t and (gu.numel() // gu.shape[-1]) % 8 == 0:
                dgu, dgut = _ext().swiglu_packed_bwd(dy.contiguous(), gu, transposed=True)
                setattr(dgu, _WGRAD_T, dgut)
                return dgu, None
            return _ext().swiglu_packed_bwd(dy.contiguous(), gu), None
        F = gu.shape[-1] // 2
        g = gu[..., :F].float()
        u = gu[..., F:].float()
        d = dy.float()
        sig = torch.sigmoid(g)
        dgate = d * u * sig * (1 + g * (1 - sig))
        dup = _swiglu_dup(d, g, sig)
        return torch.cat([dgate, dup], dim=-1).to(gu.dtype), None


def swiglu_packed(gu: torch.Tensor) -> torch.Tensor:
    return _SwiGLUPacked.apply(gu, getattr(gu, _WGRAD_WANTS_T, False))


# ---------------------------------------------------------------------------
# Fused cross-entropy (mean over non-ignored tokens)
# ---------------------------------------------------------------------------
class _FusedCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: torch.Tensor, target: torch.Tensor, ignore_index: int):
        n_tok = (target != ignore_index).sum().clamp(min=1)
        if _use_hip(logits):
            lg, tg = logits.contiguous(), target.contiguous()
            loss, lse = _ext().ce_fwd(lg, tg, ignore_index)
            ctx.save_for_backward(lg, tg, lse, n_tok)
            ctx.ignore_index = ignore_index
            ctx.hip = True
            return loss.sum() / n_tok.to(loss.dtype)
        xf = logits.float()
        lse = torch.logsumexp(xf, dim=-1)
        valid = target != ignore_index
        tgt = target.clamp(min=0)
        xt = xf.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
        loss = torch.where(valid, lse - xt, torch.zeros_like(lse))
        ctx.save_for_backward(logits, target, lse, n_tok)
        ctx.ignore_index = ignore_index
        ctx.hip = False
        return loss.sum() / n_tok.to(loss.dtype)

    @staticmethod
    def backward(ctx, dloss: torch.Tensor):
        logits, target, lse, n_tok = ctx.saved_tensors
        scale = (dloss / n_tok.to(dloss.dtype)).float()
        if ctx.hip:
            drow = scale.expand(lse.shape[0]).contiguous()
            dlogits = _ext().ce_bwd(
                logits, target, lse, drow, ctx.ignore_index, False
            )
            return dlogits, None, None
        xf = logits.float()
        p = torch.exp(xf - lse.unsqueeze(-1))
        valid = (target != ctx.ignore_index).unsqueeze(-1)
        tgt = target.clamp(min=0)
        p.scatter_add_(
            -1, tgt.unsqueeze(-1), -torch.ones_like(tgt, dtype=p.dtype).unsqueeze(-1)
        )
        d = (p * scale * valid).to(logits.dtype)
        return d, None, None


def fused_cross_entropy(
    logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -100
) -> torch.Tensor:
    """logits [N, V] (any leading dims flattened by caller), target [N]."""
    return _FusedCE.apply(logits, target, ignore_index)


# ---------------------------------------------------------------------------
# Vocab-parallel cross-entropy: every rank holds columns
# [vocab_start, vocab_start + n) of the logits (ce_vp_fwd_bf16 /
# ce_vp_bwd_bf16 in ops/csrc/cross_entropy.hip).
# ---------------------------------------------------------------------------
def _vp_hip(logits_local: torch.Tensor, *others) -> bool:
    return (
        logits_local.dtype == torch.bfloat16
        and logits_local.shape[-1] > 0
        and logits_local.shape[-1] % 8 == 0
        and _use_hip(logits_local, *others)
    )


def _vp_hit(target, vocab_start, n, ignore_index):
    """Rows whose target is a column of this shard, and that column."""
    hit = (target != ignore_index) & (target >= vocab_start) & (target < vocab_start + n)
    return hit, torch.where(hit, target - vocab_start, torch.zeros_like(target))


def _vp_check(logits_local, target, vocab_start, vocab_total):
    n = logits_local.shape[-1]
    if logits_local.dim() != 2 or target.shape != logits_local.shape[:1]:
        raise ValueError(
            f"vocab-parallel CE takes logits_local [N, n] and target [N], got "
            f"{tuple(logits_local.shape)} and {tuple(target.shape)}")
    if vocab_start < 0 or vocab_start + n > vocab_total:
        raise ValueError(
            f"shard columns [{vocab_start}, {vocab_start + n}) are not inside "
            f"the vocabulary [0, {vocab_total})")


@torch.no_grad()
def vp_ce_partials(logits_local, target, vocab_start: int, vocab_total: int,
                   ignore_index: int = -100):
    """One shard's share of the cross-entropy: (picked, lse_local), fp32 [N].

    lse_local is the log-sum-exp over the shard's n columns.  picked is the
    target's raw logit where the target is not ignore_index and lies in
    [vocab_start, vocab_start + n), else exactly 0; a target outside
    [0, vocab_total) is in no shard.  HIP for bf16 on the GPU with
    n % 8 == 0, the fp32 torch reference otherwise."""
    _vp_check(logits_local, target, vocab_start, vocab_total)
    if _vp_hip(logits_local, target):
        picked, lse_local = _ext().ce_fwd(
            logits_local.contiguous(), target.contiguous(), ignore_index,
            vocab_start=vocab_start, vocab_total=vocab_total)
        return picked, lse_local
    xf = logits_local.to(torch.promote_types(logits_local.dtype, torch.float32))
    hit, col = _vp_hit(target, vocab_start, xf.shape[-1], ignore_index)
    xt = xf.gather(-1, col.unsqueeze(-1)).squeeze(-1)
    return torch.where(hit, xt, torch.zeros_like(xt)), torch.logsumexp(xf, dim=-1)


@torch.no_grad()
def vp_ce_grad(logits_local, target, lse, drow, vocab_start: int, vocab_total: int,
               ignore_index: int = -100, inplace: bool = False):
    """dlogits[r, c] = drow[r] * (exp(x[r, c] - lse[r]) - [c + vocab_start ==
    target[r]]) in logits_local's dtype; lse is the GLOBAL log-sum-exp and
    drow counts as 0 on ignored rows.  inplace overwrites logits_local (HIP
    path: no second [N, n] buffer)."""
    _vp_check(logits_local, target, vocab_start, vocab_total)
    if _vp_hip(logits_local, target, lse, drow):
        lg = logits_local.contiguous()
        out = _ext().ce_bwd(
            lg, target.contiguous(), lse.float().contiguous(),
            drow.float().contiguous(), ignore_index, inplace,
            vocab_start=vocab_start, vocab_total=vocab_total)
        if inplace and lg is not logits_local:
            logits_local.copy_(out)
            return logits_local
        return out
    xf = logits_local.to(torch.promote_types(logits_local.dtype, torch.float32))
    hit, col = _vp_hit(target, vocab_start, xf.shape[-1], ignore_index)
    p = torch.exp(xf - lse.to(xf.dtype).unsqueeze(-1))
    p.scatter_add_(-1, col.unsqueeze(-1), -hit.to(p.dtype).unsqueeze(-1))
    scale = torch.where(target != ignore_index, drow.to(p.dtype), torch.zeros_like(drow, dtype=p.dtype))
    d = (p * scale.unsqueeze(-1)).to(logits_local.dtype)
    if inplace:
        logits_local.copy_(d)
        return logits_local
    return d


class _VocabParallelCE(torch.autograd.Function):
    """One node: partials -> (max, sum) all-reduces -> loss; backward is the
    gradient kernel alone, no collective."""

    @staticmethod
    def forward(ctx, logits_local, target, vocab_start, vocab_total, group,
                ignore_index, reduction):
        picked, lse_local = vp_ce_partials(
            logits_local, target, vocab_start, vocab_total, ignore_index)
        if group is not None and torch.distributed.get_world_size(group) > 1:
            m = lse_local.clone()
            torch.distributed.all_reduce(
                m, op=torch.distributed.ReduceOp.MAX, group=group)
            # a row that is -inf on every shard keeps exp() finite
            m = torch.where(m == float("-inf"), torch.zeros_like(m), m)
            both = torch.stack([torch.exp(lse_local - m), picked])
            torch.distributed.all_reduce(both, group=group)
            lse, picked = m + torch.log(both[0]), both[1]
        else:
            lse = lse_local
        valid = target != ignore_index
        rows = torch.where(valid, lse - picked, torch.zeros_like(lse))
        n_tok = valid.sum().clamp(min=1)
        ctx.save_for_backward(logits_local, target, lse, n_tok)
        ctx.args = (vocab_start, vocab_total, ignore_index, reduction)
        if reduction == "none":
            return rows
        return rows.sum() / n_tok.to(rows.dtype)

    @staticmethod
    def backward(ctx, dloss):
        logits_local, target, lse, n_tok = ctx.saved_tensors
        vocab_start, vocab_total, ignore_index, reduction = ctx.args
        if reduction == "none":
            drow = dloss.to(lse.dtype).contiguous()
        else:
            drow = (dloss / n_tok.to(dloss.dtype)).to(lse.dtype).expand(lse.shape[0]).contiguous()
        d = vp_ce_grad(logits_local, target, lse, drow, vocab_start, vocab_total,
                       ignore_index)
        return d, None, None, None, None, None, None


def vocab_parallel_cross_entropy(
    logits_local: torch.Tensor, target: torch.Tensor, vocab_start: int,
    vocab_total: int, group=None, ignore_index: int = -100,
    reduction: str = "mean",
) -> torch.Tensor:
    """Cross-entropy over class-sharded logits: logits_local [N, n] holds
    columns [vocab_start, vocab_start + n) of a vocab_total-class row on
    this rank of `group`, target [N] the global class ids (the same on every
    rank).  The forward makes two all-reduces over `group`, on fp32 fields of
    N (max) and 2N (sum) elements; the backward makes none.  reduction:
    "mean" over the non-ignored targets (count clamped to 1) or "none" (the
    per-row vector, 0 on ignored rows).  group=None is the one-shard case:
    with vocab_start=0 and vocab_total=n it is fused_cross_entropy's loss."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"reduction must be 'mean' or 'none', got {reduction!r}")
    return _VocabParallelCE.apply(
        logits_local, target, int(vocab_start), int(vocab_total), group,
        int(ignore_index), reduction)


# ---------------------------------------------------------------------------
# Tuned flash attention: our CDNA4 MFMA forward (ops/csrc/attention_fwd.hip,
# returns logsumexp) + backward (ops/csrc/attention_bwd2.hip); causal,
# head_dim 128, GQA, seq % 256 == 0; optionally the packed-document mask of
# flash_attention(..., contiguous_segments=True).  _FlashAttentionLse below
# runs the same family without a mask (Sq != Sk allowed) and with a
# differentiable lse.
# ---------------------------------------------------------------------------
class _FlashAttention(torch.autograd.Function):
    """Causal flash attention, fully on our MFMA kernels: fa_fwd
    (attention_fwd.hip, ~565 TF at the Llama-8B shape vs the stock AOTriton
    forward's ~477 TF) + fa_bwd2 (attention_bwd2.hip, ~18.7 ms vs the
    library backward's ~20.9 ms at that shape).  Set VESCALE_FA=aten to
    fall back to the torch/AOTriton kernels.

    o is produced, saved and differentiated as [B, S, H, D]: the forward
    returns its [B, H, S, D]-shaped view and the backward reads dout in the
    same layout, which removed the two transpose copies per layer (0.134 ms
    each at the Llama-8B bench shape, 64 launches per step) around the
    output projection.  fa_fwd and fa2_dq are as fast as before; fa2_dv and
    fa2_dk stage dO rows that are now 8 KiB apart and cost 0.13-0.19 ms more
    per layer between them, so the net is about -0.1 ms per layer
    (profiles/streaming_kernels_r3.txt)."""

    @staticmethod
    def forward(ctx, q, k, v, scale, seg_ids=None):
        # q,k,v: [B, H, S, D] contiguous bf16.  The kernel writes o as
        # [B, S, H, D], the layout the output projection reads; callers get
        # the [B, H, S, D]-shaped view of it.
        # seg_ids [B, S] int32 contiguous: packed documents as runs of equal
        # ids.  fa_fwd derives the run bounds [B, 2, S] once and hands them
        # back; they are saved for fa_bwd2's SEG kernels.
        if seg_ids is None:
            out, lse = _ext().fa_fwd(q, k, v, scale, out_bshd=True)
            bounds = None
        else:
            out, lse, bounds = _ext().fa_fwd(q, k, v, scale, out_bshd=True,
                                             segment_ids=seg_ids)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.bounds = bounds
        ctx.scale = scale
        return out.transpose(1, 2)

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        if ctx.bounds is not None:
            # the fused dv+dk kernel has no segment mask: always the split ones
            dout = dout.transpose(1, 2)
            if not dout.is_contiguous():
                dout = dout.contiguous()
            dq, dk, dv = _ext().fa_bwd2(q, k, v, out, dout, lse, ctx.scale, False,
                                        bshd=True, seg_bounds=ctx.bounds)
            return dq, dk, dv, None, None
        # default OFF: the fused dv+dk kernel is numerically exact but
        # measured SLOWER (whole bwd 17.9 ms vs 11.2 ms at B4 H32/8 S8192,
        # profiles/fa_fused_dvdk_ab_r2.log) — its 2-accumulator register set
        # only fits at 1 wave/SIMD (4-wave blocks), and the lost latency
        # hiding outweighs the deduplicated ST GEMM + staging.  Kept for A/B;
        # it reads [B, H, S, D] only.
        fused = os.environ.get("VESCALE_FA_FUSED_DVDK", "0") == "1"
        if fused:
            dq, dk, dv = _ext().fa_bwd2(
                q, k, v, out.transpose(1, 2).contiguous(), dout.contiguous(), lse,
                ctx.scale, True)
            return dq, dk, dv, None, None
        # the gradient of the [B, H, S, D] view of a [B, S, H*D] consumer is
        # contiguous once transposed back: no copy on the model's path
        dout = dout.transpose(1, 2)
        if not dout.is_contiguous():
            dout = dout.contiguous()
        dq, dk, dv = _ext().fa_bwd2(q, k, v, out, dout, lse, ctx.scale, False, bshd=True)
        return dq, dk, dv, None, None


# VESCALE_FA_FULL selects where flash_attention sends the D=128 calls that the
# tuned family serves beyond causal self-attention without an lse (non-causal,
# Sq != Sk, return_lse):
#   tuned  the 32x32 kernels: FULL instantiations, fa_bwd_preprocess_dlse
#   gen    the general 16x16 kernels (attention_gen.hip), as before: A/B, fallback
# The default follows tools/fa_full_bench.py (profiles/fa32_full.txt): tuned is
# the default only while it beats gen at all three shapes measured there.
FA_FULL_DEFAULT = "tuned"


def _fa_full_backend():
    backend = os.environ.get("VESCALE_FA_FULL", FA_FULL_DEFAULT)
    if backend not in ("tuned", "gen"):
        raise ValueError(f"VESCALE_FA_FULL = {backend!r} must be 'tuned' or 'gen'")
    return backend


class _FlashAttentionLse(torch.autograd.Function):
    """The tuned D=128 kernels with two differentiable outputs (out, lse),
    [B, H, S, D] throughout: fa_fwd / fa_bwd2 with causal=False (the FULL
    kernels: no mask, k/v of their own length Sk) or causal=True (the causal
    kernels _FlashAttention runs, here with the lse handed out).  The lse's
    cotangent reaches the kernels through the delta pre-pass (dS = P * (dP -
    (delta - dlse))); a missing dout is zeros, a missing dlse no dlse."""

    @staticmethod
    def forward(ctx, q, k, v, scale, causal):
        out, lse = _ext().fa_fwd(q, k, v, scale, causal=causal)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.args = (scale, causal)
        ctx.set_materialize_grads(False)
        return out, lse

    @staticmethod
    def backward(ctx, dout, dlse):
        q, k, v, out, lse = ctx.saved_tensors
        scale, causal = ctx.args
        dout = torch.zeros_like(out) if dout is None else dout.contiguous()
        if dlse is not None:
            dlse = dlse.float().contiguous()
        dq, dk, dv = _ext().fa_bwd2(q, k, v, out, dout, lse, scale, False,
                                    causal=causal, dlse=dlse)
        return dq, dk, dv, None, None


def flash_attention_causal(q, k, v):
    """Causal flash attention, [B,H,S,D] bf16; GQA via Hkv < Hq.  Falls back
    to torch SDPA off-GPU / without the extension loudly on GPU.

    On the HIP path the result is a [B,H,S,D]-shaped VIEW of a contiguous
    [B,S,H,D] tensor (not contiguous itself): o.transpose(1, 2).reshape(B, S,
    H*D), what an output projection wants, is a view too."""
    import math

    scale = 1.0 / math.sqrt(q.shape[-1])
    if (
        _use_hip(q, k, v)
        and q.shape[-1] == 128
        and q.shape[2] % 256 == 0
        and os.environ.get("VESCALE_FA", "hip") == "hip"
    ):
        return _FlashAttention.apply(
            q.contiguous(), k.contiguous(), v.contiguous(), scale
        )
    return torch.nn.functional.scaled_dot_product_attention(
        q, k, v, is_causal=True, enable_gqa=q.shape[1] != k.shape[1]
    )


# ---------------------------------------------------------------------------
# General-shape flash attention with a differentiable LSE
# (ops/csrc/attention_gen.hip): any Sq/Sk, D in {64,128}, MHA/GQA/MQA,
# optional causal mask  j <= i + causal_shift.
# ---------------------------------------------------------------------------
def _attention_ref(q, k, v, is_causal, shift, scale, dtype=None, *, q_seg=None,
                   kv_seg=None, lower=None):
    """Differentiable torch attention returning (out, lse): the CPU path and
    the oracle of the general kernel.  Matmuls and softmax run in `dtype`
    (default: fp32, or q's dtype if wider); GQA by head grouping; key j is
    visible to query i iff j <= i + shift and, with q_seg [B,Sq] / kv_seg
    [B,Sk] given, kv_seg[b, j] == q_seg[b, i] and, with `lower` given,
    j >= i + lower; a row with no visible key gives out = 0, lse = -inf and
    zero gradients."""
    if dtype is None:
        dtype = torch.promote_types(q.dtype, torch.float32)
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    qg = q.to(dtype).reshape(B, Hkv, Hq // Hkv, Sq, D)
    s = (qg @ k.to(dtype).unsqueeze(2).transpose(-1, -2)) * scale
    i = torch.arange(Sq, device=q.device).unsqueeze(1)
    j = torch.arange(Sk, device=q.device).unsqueeze(0)
    if is_causal:
        s = s.masked_fill(j > i + shift, float("-inf"))
    if lower is not None:
        s = s.masked_fill(j < i + lower, float("-inf"))
    if q_seg is not None:
        other = q_seg.unsqueeze(2) != kv_seg.unsqueeze(1)       # [B, Sq, Sk]
        s = s.masked_fill(other[:, None, None], float("-inf"))
    m = s.detach().amax(-1, keepdim=True)
    m = torch.where(m == float("-inf"), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    dead = l == 0
    l1 = torch.where(dead, torch.ones_like(l), l)
    out = (e / l1) @ v.to(dtype).unsqueeze(2)
    lse = torch.where(dead, torch.full_like(l, float("-inf")), m + torch.log(l1))
    lse_dtype = torch.promote_types(q.dtype, torch.float32)
    return (out.reshape(B, Hq, Sq, D).to(q.dtype),
            lse.reshape(B, Hq, Sq).to(lse_dtype))


class _FlashAttentionGen(torch.autograd.Function):
    """fa_gen_fwd / fa_gen_bwd: one node with two differentiable outputs.
    q_seg / kv_seg (contiguous int32 [B,Sq] / [B,Sk], or both None) are
    non-differentiable inputs; backward hands the ids themselves to
    fa_gen_bwd, which derives its tile bounds again.  lower (int or None):
    the window's bound j >= i + lower, the WIN kernels."""

    @staticmethod
    def forward(ctx, q, k, v, scale, causal, shift, q_seg=None, kv_seg=None,
                lower=None):
        out, lse = _ext().fa_gen_fwd(q, k, v, scale, causal, shift,
                                     q_seg=q_seg, kv_seg=kv_seg, lower=lower)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.args = (scale, causal, shift, lower)
        ctx.seg = (q_seg, kv_seg)
        ctx.set_materialize_grads(False)
        return out, lse

    @staticmethod
    def backward(ctx, dout, dlse):
        q, k, v, out, lse = ctx.saved_tensors
        scale, causal, shift, lower = ctx.args
        q_seg, kv_seg = ctx.seg
        dout = torch.zeros_like(out) if dout is None else dout.contiguous()
        if dlse is not None:
            dlse = dlse.float().contiguous()
        dq, dk, dv = _ext().fa_gen_bwd(
            q, k, v, out, dout, lse, dlse, scale, causal, shift,
            q_seg=q_seg, kv_seg=kv_seg, lower=lower
        )
        return dq, dk, dv, None, None, None, None, None, None


def _segment_args(q_segment_ids, kv_segment_ids, B, Sq, Sk):
    """flash_attention's segment-id rules: (q_seg, kv_seg) as contiguous
    int32 [B,Sq] / [B,Sk], or (None, None)."""
    if q_segment_ids is None and kv_segment_ids is None:
        return None, None
    if q_segment_ids is None:
        raise ValueError("kv_segment_ids given without q_segment_ids")
    if kv_segment_ids is None:
        if Sq != Sk:
            raise ValueError(
                f"kv_segment_ids is required when Sq != Sk ({Sq} != {Sk})")
        kv_segment_ids = q_segment_ids
    out = []
    for name, t, S in (("q_segment_ids", q_segment_ids, Sq),
                       ("kv_segment_ids", kv_segment_ids, Sk)):
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError(f"{name} must have an integer dtype, got {t.dtype}")
        if tuple(t.shape) != (B, S):
            raise ValueError(f"{name} must be [B, S] = [{B}, {S}], got {list(t.shape)}")
        out.append(t.to(torch.int32).contiguous())
    return out[0], out[1]


def _window_args(window, is_causal, causal_shift):
    """flash_attention's window rules: the kernels' (causal, shift, lower)
    for window = (left, right) around the diagonal d(i) = i + causal_shift.
    An upper bound is what (causal, shift) already express, so `right` is
    folded into them; only lower = causal_shift - left is new."""
    if not isinstance(window, (tuple, list)) or len(window) != 2:
        raise ValueError(f"window must be a pair (left, right), got {window!r}")
    for side, w in zip(("left", "right"), window):
        if w is None:
            continue
        if isinstance(w, bool) or not isinstance(w, int):
            raise ValueError(f"window {side} must be an int or None, got {w!r}")
        if w < 0:
            raise ValueError(f"window {side} must be >= 0, got {w}")
    left, right = window
    lower = None if left is None else causal_shift - left
    if is_causal:
        return True, causal_shift, lower     # j <= d(i) already implies right
    if right is None:
        return False, 0, lower
    return True, causal_shift + right, lower


def segment_ids_from_cu_seqlens(cu_seqlens, total: int) -> torch.Tensor:
    """Segment ids [total] (int32) of a packed row from the varlen
    convention: cu_seqlens = [0, e_0, e_1, ...] (non-decreasing), document d
    covering positions [cu_seqlens[d], cu_seqlens[d + 1]).  Positions past
    cu_seqlens[-1] (padding) get one id of their own, so padding attends
    only to padding."""
    cu = torch.as_tensor(cu_seqlens)
    if cu.dim() != 1 or cu.numel() < 1:
        raise ValueError("cu_seqlens must be a non-empty 1-D sequence")
    if cu.dtype.is_floating_point or cu.dtype == torch.bool:
        raise ValueError(f"cu_seqlens must have an integer dtype, got {cu.dtype}")
    if int(cu[-1]) > total:
        raise ValueError(f"cu_seqlens[-1] = {int(cu[-1])} is past total = {total}")
    pos = torch.arange(total, device=cu.device)
    # id = number of document ends at or before the position: document d has
    # d ends before it, the padding tail len(cu) - 1 of them
    ids = torch.searchsorted(cu[1:].to(torch.int64).contiguous(), pos, right=True)
    return ids.to(torch.int32)


def _run_start_ids(ids):
    """ids [B, S] -> int32 [B, S], every position's id replaced by the first
    position of its maximal run of equal ids: equal run start <=> same run, so
    the equality mask over the result is the run mask.  A boundary flag and a
    running maximum on the ids' device; no host sync."""
    S = ids.shape[1]
    pos = torch.arange(S, device=ids.device, dtype=torch.int32).expand_as(ids)
    edge = torch.ones_like(ids, dtype=torch.bool)
    edge[:, 1:] = ids[:, 1:] != ids[:, :-1]
    return torch.cummax(torch.where(edge, pos, torch.zeros_like(pos)), dim=1).values


def flash_attention(q, k, v, *, is_causal=False, causal_shift=0, scale=None,
                    return_lse=False, q_segment_ids=None, kv_segment_ids=None,
                    contiguous_segments=False, window=None):
    """Attention over q [B,Hq,Sq,D], k/v [B,Hkv,Sk,D] (Hq % Hkv == 0).

    With is_causal, key j is visible to query i iff j <= i + causal_shift
    (0: top-left triangle; Sk - Sq: bottom-right alignment).  A query row
    with no visible key yields out = 0, lse = -inf and zero gradients.
    Returns out, or (out, lse) with lse [B,Hq,Sq] fp32 (natural log) when
    return_lse; both outputs are differentiable.

    Sliding window (local attention): window = (left, right), each a
    non-negative int or None (unbounded on that side), around the diagonal
    d(i) = i + causal_shift: key j is visible to query i iff, in addition to
    every other rule, j >= d(i) - left and j <= d(i) + right.  With is_causal,
    right adds nothing; is_causal=True with window=(W - 1, 0) is the
    sliding_window = W of Mistral-style models.  causal_shift is allowed
    without is_causal when a window is given (Sk - Sq: a bottom-right aligned
    band).  A row the window leaves with no key is a dead row as above.  Bad
    windows (negative or non-int entries, not a pair) raise ValueError.  The
    general kernels skip the key tiles left of the band and the query tiles
    below it, so the work is O(S * W), not O(S^2).

    Packed sequences: with q_segment_ids [B,Sq] and kv_segment_ids [B,Sk]
    (any integer dtype) key j is visible to query i iff, in addition,
    kv_segment_ids[b, j] == q_segment_ids[b, i].  Ids are compared for
    equality only: no value is special and they need not be sorted.
    kv_segment_ids may be left out when Sq == Sk (the same ids for both);
    otherwise both are required (ValueError).  A query whose id no visible
    key carries is a dead row as above; a key no query sees gets zero dk/dv.
    segment_ids_from_cu_seqlens builds ids from document boundaries.

    contiguous_segments=True is the promise that documents are contiguous:
    the mask is then defined by the MAXIMAL RUNS of equal ids along the
    sequence, per batch row: key j is visible to query i iff both lie in the
    same run and j <= i.  For ids from segment_ids_from_cu_seqlens that is
    the equality mask above.  An id that reappears after its run ended starts
    a new document (defined behaviour, not an error).  It needs q_segment_ids,
    is_causal=True, causal_shift == 0, Sq == Sk and no kv_segment_ids
    (ValueError otherwise).  Every path gives this answer: the tuned D=128
    kernels mask by run bounds; everywhere else the ids are replaced on the
    device by their run's first position and go to the general kernel or the
    reference unchanged.  VESCALE_FA_SEG=gen keeps such calls off the tuned
    kernels (A/B).

    Dispatch: (1) the tuned D=128 causal kernels when their gate holds, no
    lse is wanted and there are no segment ids, or the ids come with
    contiguous_segments, and there is no window (the tuned kernels have no
    band mask: a call with a window never takes them); (1b) the same family
    for bf16 on GPU with D == 128, no window (or one that masks nothing
    beyond is_causal: left >= Sq - 1 + causal_shift and right folded into
    is_causal, so that a neutral window gives the bits of no window), no
    segment ids and Sq and Sk
    positive multiples of 256: any call without is_causal (the FULL kernels:
    no mask, Sq and Sk independent, with or without return_lse), and
    is_causal with causal_shift == 0, Sq == Sk and return_lse (the causal
    kernels, lse handed out and differentiable); VESCALE_FA_FULL=gen keeps
    these calls on the general kernels (A/B, fallback); (2) the general HIP
    kernel for bf16 on GPU with D in {64, 128}: shifted causal masks, windows,
    segment ids without contiguous_segments (and with it when an lse is
    wanted), D = 64, ragged lengths; (3) the torch reference (CPU, other
    dtypes / head dims, VESCALE_FA=aten)."""
    import math

    if window is not None:
        causal, shift, lower = _window_args(window, bool(is_causal), int(causal_shift))
    elif causal_shift != 0 and not is_causal:
        raise ValueError("causal_shift != 0 requires is_causal=True")
    else:
        causal, shift, lower = bool(is_causal), int(causal_shift), None
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    if contiguous_segments:
        if q_segment_ids is None:
            raise ValueError("contiguous_segments=True requires q_segment_ids")
        if kv_segment_ids is not None:
            raise ValueError("contiguous_segments=True takes no kv_segment_ids: "
                             "the documents of q and k/v are the same runs")
        if not is_causal or causal_shift != 0 or Sq != Sk:
            raise ValueError("contiguous_segments=True requires is_causal=True, "
                             f"causal_shift == 0 and Sq == Sk (got is_causal={is_causal}, "
                             f"causal_shift={causal_shift}, Sq={Sq}, Sk={Sk})")
    q_seg, kv_seg = _segment_args(q_segment_ids, kv_segment_ids, B, Sq, Sk)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    hip = (
        os.environ.get("VESCALE_FA", "hip") == "hip"
        and all(t.is_cuda and t.dtype == torch.bfloat16 for t in (q, k, v))
        and D in (64, 128)
        and Hq % Hkv == 0
        and _use_hip(q, k, v)
    )
    if (hip and not return_lse and window is None and is_causal and causal_shift == 0
            and Sq == Sk and D == 128 and Sq % 256 == 0
            and (q_seg is None or (contiguous_segments and
                                   os.environ.get("VESCALE_FA_SEG", "tuned") != "gen"))):
        return _FlashAttention.apply(
            q.contiguous(), k.contiguous(), v.contiguous(), scale, q_seg
        )
    # the tuned family beyond that: no mask at all with any two lengths (the
    # FULL kernels), or the causal kernels with the lse handed out.  By the
    # mask, not by its spelling: (causal, shift, lower) are the kernels' own
    # terms, and a lower bound j >= i + lower that no pair (i, j) violates
    # (left >= Sq - 1 + shift) is no band, so such a call is, bit for bit, the
    # call without a window.
    no_band = lower is None or lower <= -(Sq - 1)
    if (hip and D == 128 and no_band and q_seg is None
            and Sq > 0 and Sk > 0 and Sq % 256 == 0 and Sk % 256 == 0
            and (not causal or (shift == 0 and Sq == Sk and return_lse))
            and _fa_full_backend() == "tuned"):
        out, lse = _FlashAttentionLse.apply(
            q.contiguous(), k.contiguous(), v.contiguous(), float(scale), causal)
        return (out, lse) if return_lse else out
    if contiguous_segments:
        q_seg = kv_seg = _run_start_ids(q_seg)
    if hip:
        out, lse = _FlashAttentionGen.apply(
            q.contiguous(), k.contiguous(), v.contiguous(), float(scale),
            causal, shift, q_seg, kv_seg, lower,
        )
    else:
        out, lse = _attention_ref(q, k, v, causal, shift, scale,
                                  q_seg=q_seg, kv_seg=kv_seg, lower=lower)
    return (out, lse) if return_lse else out


# ---------------------------------------------------------------------------
# flat AdamW + grad utilities (no autograd)
# ---------------------------------------------------------------------------
@torch.no_grad()
def adamw_step_flat(
    param_bf16: torch.Tensor,
    master_f32: Optional[torch.Tensor],
    grad: torch.Tensor,
    m: torch.Tensor,
    v: torch.Tensor,
    *,
    lr: float,
    beta1: float = 0.9,
    beta2: float = 0.95,
    eps: float = 1e-8,
    weight_decay: float = 0.0,
    step: int = 1,
    grad_scale: float = 1.0,
    clip_scale: Optional[torch.Tensor] = None,
):
    if _use_hip(param_bf16, grad, m, v):
        _ext().adamw_step(
            param_bf16, master_f32, grad, m, v, lr, beta1, beta2, eps,
            weight_decay, step, grad_scale, clip_scale,
        )
        return
    g = grad.float() * grad_scale
    if clip_scale is not None:
        g = g * clip_scale.item()
    p = master_f32 if master_f32 is not None else param_bf16.float()
    p.mul_(1 - lr * weight_decay)
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1**step
    bc2 = 1 - beta2**step
    denom = (v / bc2).sqrt().add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)
    param_bf16.copy_(p.to(param_bf16.dtype))


@torch.no_grad()
def l2norm_sq(x: torch.Tensor) -> torch.Tensor:
    if _use_hip(x):
        return _ext().l2norm_sq(x.contiguous()).squeeze(0)
    return x.float().pow(2).sum()


@torch.no_grad()
def scale_flat_(x: torch.Tensor, scale) -> None:
    if _use_hip(x):
        if isinstance(scale, torch.Tensor):
            _ext().scale_(x, scale.float().contiguous(), 1.0)
        else:
            _ext().scale_(x, None, float(scale))
        return
    if isinstance(scale, torch.Tensor):
        # like the kernel: an fp32 product by the fp32 scale, rounded once
        x.copy_((x.float() * scale.float()).to(x.dtype))
    else:
        x.mul_(scale)


# ---------------------------------------------------------------------------
# Linear (in-tree CDNA4 GEMM path)
# ---------------------------------------------------------------------------
# VESCALE_GEMM selects the nn.Linear GEMM backend:
#   "blaslt" (default) — torch.matmul -> hipBLASLt Tensile assembly kernels;
#                        forward and dgrad as F.linear issues them, wgrad in
#                        the operand layout _wgrad_form picks per shape, its
#                        transposed operands made by ops/csrc/transpose.hip.
#   "gemm8"            — the in-tree 256x256 8-phase MFMA kernel
#                        (ops/csrc/gemm8.hip, rot3np schedule) for the
#                        forward and dgrad GEMMs; its wgrad is the library's
#                        dy.t() @ x, form (a) of the wgrad forms below (the
#                        layout rule of linear() belongs to the blaslt
#                        backend): the
#                        contraction-major kernels that exist now are the
#                        grouped expert forms below (gemm_grouped.hip, dgrad
#                        and wgrad staged transposed into LDS), which serve
#                        grouped_linear, not this dense path.  Honest A/B:
#                        profiles/gemm8_variants_ab_r2.log — the in-tree
#                        kernel is ~75% of hipBLASLt on Llama shapes, so
#                        blaslt remains the default (VERDICT r1 item 1:
#                        "do not ship a regression").
#   "fp8"              — opt-in 8-bit linear (_LinearFp8 below): forward,
#                        dgrad and wgrad all run the in-tree fp8 GEMM
#                        (ops/csrc/gemm_fp8.hip) on operands quantised by its
#                        amax / cast kernels; e4m3 for x and w, e5m2 for dy,
#                        per-tensor current scaling (no amax history), bf16
#                        results.  Shapes outside M, N, K % 256 == 0, a bias,
#                        a non-bf16 or CPU tensor fall back to F.linear per
#                        call.  A/B: profiles/gemm_fp8_ab.txt; the default
#                        stays blaslt.
# Reference parity: sharded matmul family, SURVEY.md §2.7;
# legacy/vescale/dtensor/ops/matrix_ops.py:113.
def _gemm_backend() -> str:
    return os.environ.get("VESCALE_GEMM", "blaslt")


def _g8_ok(m: int, n: int, k: int) -> bool:
    return m % 256 == 0 and n % 256 == 0 and k % 64 == 0


class _Linear8(torch.autograd.Function):
    """y = x @ w^T via the in-tree TN kernel; dgrad = gemm_tn(dy, w^T)
    (one cheap [N,K]->[K,N] transpose per backward — arithmetic intensity
    of the GEMM is ~4 orders above the copy); wgrad is the library's
    dy.t() @ x (form "a" of WGRAD_FORMS)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor):
        ctx.save_for_backward(x, w)
        xs = x.shape
        x2 = x.reshape(-1, xs[-1])
        m, k = x2.shape
        n = w.shape[0]
        if x.is_cuda and x.dtype == torch.bfloat16 and _g8_ok(m, n, k):
            y = _ext().gemm_tn8(x2.contiguous(), w.contiguous(), 4)
        else:
            y = x2 @ w.t()
        return y.reshape(*xs[:-1], n)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w = ctx.saved_tensors
        dys = dy.reshape(-1, dy.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        m, n = dys.shape
        k = w.shape[1]
        dx = dw = None
        if ctx.needs_input_grad[0]:
            if dy.is_cuda and dy.dtype == torch.bfloat16 and _g8_ok(m, k, n):
                wt = w.t().contiguous()
                dx = _ext().gemm_tn8(dys.contiguous(), wt, 4)
            else:
                dx = dys @ w
            dx = dx.reshape(x.shape)
        if ctx.needs_input_grad[1]:
            dw = dys.t() @ x2  # library wgrad, form "a" (see header note)
        return dx, dw


# ---------------------------------------------------------------------------
# FP8 linear (VESCALE_GEMM=fp8): ops/csrc/gemm_fp8.hip
# ---------------------------------------------------------------------------
# The fp8 GEMM is TN: C[M,N] = A[M,K] . B[N,K]^T with K innermost on both
# operands, B always e4m3.  The three products of a linear therefore need
#   forward  y  = gemm(xq  [M,K], wq  [N,K])
#   dgrad    dx = gemm(dyq [M,N], wq^T [K,N])
#   wgrad    dw = gemm(dyq^T [N,M], xq^T [K,M])
# so x, w and dy are each quantised ONCE into both layouts (one amax pass, one
# cast pass that reads the bf16 tensor once and writes q and q^T).  Scaling is
# per tensor and current: scale = amax / fmt_max, floored at the smallest
# normal fp32 so that an all-zero tensor gives q = 0; it stays on the device
# (1-element ops on the amax kernel's output, no host sync, capturable).
# The context keeps xq^T, wq^T and the two scales: no bf16 x, so the
# activation kept for backward is half the bf16 path's.
# Contract: M, N, K multiples of 256 (each is a tile extent of one product
# and the contraction of another).  The LM head stays on the bf16 path: its
# dy and dy^T copies would be transients of M * vocab bytes each, so the path
# takes the bound of _wgrad_form on that transient, 2 M N <= 2^31, and the
# logits keep bf16 operands.
_FP8_MAX = {torch.float8_e4m3fn: 448.0, torch.float8_e5m2: 57344.0}
_F32_TINY = torch.finfo(torch.float32).tiny


def _fp8_fits(x: torch.Tensor, w: torch.Tensor) -> bool:
    if not (x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.dim() == 2
            and x.dim() >= 2 and x.shape[-1] == w.shape[1] and _use_hip(x, w)):
        return False
    n, k = w.shape
    m = x.numel() // k if k else 0
    return (m > 0 and m % 256 == 0 and n % 256 == 0 and k % 256 == 0
            and 2 * m * n <= 2 ** 31)


def _fp8_quantize(t: torch.Tensor, dtype: torch.dtype):
    """t [R,C] bf16 -> (q [R,C], q^T [C,R], scale fp32 [1]) with t ~ q * scale."""
    C = _ext()
    r, c = t.shape
    amax = C.gemm_tn8(t, [], 0, group_form="fp8_amax")
    # a tensor divisor: by a Python scalar the device kernel multiplies by the
    # reciprocal, one ulp off the division that defines the scale
    scale = amax.div_(torch.full_like(amax, _FP8_MAX[dtype])).clamp_min_(_F32_TINY)
    q = torch.empty((r, c), dtype=dtype, device=t.device)
    qt = torch.empty((c, r), dtype=dtype, device=t.device)
    C.gemm_tn8(t, [], 0, group_form="fp8_quantize", scale_a=scale, group_out=q, out_t=qt)
    return q, qt, scale


class _LinearFp8(torch.autograd.Function):
    """y = x @ w^T with all three GEMMs in fp8: x, w in e4m3, dy in e5m2."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor):
        n, k = w.shape
        xq, xqt, sx = _fp8_quantize(x.reshape(-1, k).contiguous(), torch.float8_e4m3fn)
        wq, wqt, sw = _fp8_quantize(w.contiguous(), torch.float8_e4m3fn)
        y = _ext().gemm_tn8(xq, wq, 0, scale_a=sx, scale_b=sw)
        ctx.save_for_backward(xqt, wqt, sx, sw)
        ctx.x_shape = x.shape
        return y.reshape(*x.shape[:-1], n)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        xqt, wqt, sx, sw = ctx.saved_tensors
        C = _ext()
        dyq, dyqt, sd = _fp8_quantize(dy.reshape(-1, dy.shape[-1]).contiguous(),
                                      torch.float8_e5m2)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = C.gemm_tn8(dyq, wqt, 0, scale_a=sd, scale_b=sw).reshape(ctx.x_shape)
        if ctx.needs_input_grad[1]:
            dw = C.gemm_tn8(dyqt, xqt, 0, scale_a=sd, scale_b=sx)
        return dx, dw


# ---------------------------------------------------------------------------
# Dense wgrad in the library's fast operand layout (NOTES_WGRAD_LAYOUT.md)
# ---------------------------------------------------------------------------
# dw [N,K] = dy^T [N,M] . x [M,K].  autograd's F.linear hands the library
# dy.t() @ x, both operands strided along the contraction M, the layout class
# the library runs slowest.  The same product in other operand layouts, the
# transposed operands made by the streaming transposing copy of
# ops/csrc/transpose.hip (or, for dy of w13, written by swiglu_packed_bwd as a
# second output):
#   "a"  dy.t() @ x          the form of F.linear's autograd
#   "b"  dyT @ x             dyT = dy^T contiguous [N,M]
#   "c"  dyT @ xT.t()        and xT = x^T contiguous [K,M]: both operands
#                            contiguous along the contraction, the forward's class
#   "d"  (xT @ dy)^T         the [K,N] result transposed by the same copy
WGRAD_FORMS = ("a", "b", "c", "d")

# side channel between _LinearWgrad and _SwiGLUPacked: the linear's output
# carries _WGRAD_WANTS_T, the gradient that comes back carries its transpose
_WGRAD_WANTS_T = "_vescale_wgrad_wants_t"
_WGRAD_T = "_vescale_wgrad_t"


def _wgrad_form(m: int, n: int, k: int) -> str:
    """The static rule: which form the wgrad of a [M,K] x [N,K]^T linear takes.
    Shapes only: no timing, no table read at run time, so two runs of one
    build issue the same calls.

    From profiles/wgrad_layout_ab.txt (M = 32768): the library runs (c) at
    1.4-1.6 PF/s where (a) runs at 1.0-1.2, but the transposes of dy [M,N] and
    x [M,K] cost what they move, so the change pays only where the output is
    wide against the contraction-free width of x: N >= 4K, and where dy^T is
    an affordable transient (at most 2 GiB).  That is w13: 6.4 -> 4.8 ms + 0.12
    for x^T + 0.35 in swiglu_packed_bwd for dy^T, and there the library's (c)
    kernel sums in the order of its (a) kernel: dw keeps its bits
    (profiles/wgrad_layout_bits.txt).  Below N = 4K (wqkv, wo, w2) no form
    beats (a) by more than its transposes cost.  The LM head (dy^T 8.4 GB)
    stays on (a) too: (d) would save 3 ms per step there, but the library's
    kernels for that shape sum in another order, a few dw elements in 10^5
    change, and the training run no longer reproduces the earlier one."""
    if m >= 4096 and n >= 4 * k and 2 * m * n <= 2 ** 31:
        return "c"
    return "a"


def _transposed(t: torch.Tensor) -> torch.Tensor:
    """t [R,C] bf16 -> t^T as a contiguous [C,R] (ops/csrc/transpose.hip)."""
    return _ext().gemm_tn8(t.contiguous(), [], 0, group_form="transpose")


def _wgrad_fits(x: torch.Tensor, w: torch.Tensor) -> bool:
    """What the transposing copy takes: bf16 on the GPU, every extent a
    multiple of 8 (16-byte chunks on both sides)."""
    m = x.numel() // x.shape[-1] if x.shape[-1] else 0
    return (
        x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
        and w.dim() == 2 and x.dim() >= 2 and x.shape[-1] == w.shape[1]
        and m > 0 and m % 8 == 0 and w.shape[0] % 8 == 0 and w.shape[1] % 8 == 0
        and _use_hip(x, w)
    )


class _LinearWgrad(torch.autograd.Function):
    """y = x @ w^T and dx = dy @ w are the library calls of F.linear and its
    autograd, so both keep their bits; dw takes `form`.  Nothing beyond x and
    w is saved, and every transposed operand dies in backward."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, form: str):
        ctx.save_for_backward(x, w)
        ctx.form = form
        return torch.nn.functional.linear(x, w)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w = ctx.saved_tensors
        n, k = w.shape
        dys = dy.reshape(-1, n)
        x2 = x.reshape(-1, k)
        dyt = getattr(dy, _WGRAD_T, None)
        if dyt is not None:
            delattr(dy, _WGRAD_T)
            if dyt.shape != (n, dys.shape[0]):
                dyt = None
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = (dys @ w).reshape(x.shape)
        if ctx.needs_input_grad[1]:
            form = ctx.form
            if form in ("b", "c") and dyt is None:
                dyt = _transposed(dys)
            if form == "b":
                dw = dyt @ x2
            elif form == "c":
                dw = dyt @ _transposed(x2).t()
            elif form == "d":
                dw = _transposed(_transposed(x2) @ dys)
            else:
                dw = dys.t() @ x2
        return dx, dw, None


def linear(x: torch.Tensor, w: torch.Tensor,
           bias: Optional[torch.Tensor] = None, *, _wgrad_form_override: Optional[str] = None,
           ) -> torch.Tensor:
    """F.linear; on the default backend, for bf16 GPU tensors without bias,
    with the wgrad product in the operand layout _wgrad_form picks for the
    shape.  _wgrad_form_override (tests, tools/wgrad_layout_ab.py) forces a
    form of WGRAD_FORMS."""
    backend = _gemm_backend()
    if backend == "gemm8" and bias is None:
        return _Linear8.apply(x, w)
    if backend == "fp8" and bias is None and _fp8_fits(x, w):
        return _LinearFp8.apply(x, w)
    if bias is None and x.is_cuda and _wgrad_fits(x, w):
        form = _wgrad_form_override or _wgrad_form(x.numel() // x.shape[-1], *w.shape)
        if form not in WGRAD_FORMS:
            raise ValueError(f"wgrad form must be one of {WGRAD_FORMS}, got {form!r}")
        if form != "a" or _wgrad_form_override:
            y = _LinearWgrad.apply(x, w, form)
            if form in ("b", "c"):
                setattr(y, _WGRAD_WANTS_T, True)
            return y
    return torch.nn.functional.linear(x, w, bias)


# ---------------------------------------------------------------------------
# Grouped expert linear (MoE): one launch per GEMM over all experts
# ---------------------------------------------------------------------------
GROUPED_MAX_EXPERTS = 64


def _weight_list(weights):
    """A stacked [E,N,K] tensor or a sequence of E [N,K] tensors -> (list of
    the tensors the kernels read, stacked?)."""
    if isinstance(weights, torch.Tensor):
        return [weights], True
    return list(weights), False


def grouped_fits(x: torch.Tensor, weights) -> bool:
    """The shape contract of the grouped kernels: bf16 on the GPU, 1..64
    experts, N and K multiples of 128."""
    ws, stacked = _weight_list(weights)
    if not ws or (stacked and ws[0].dim() != 3):
        return False
    n_exp = ws[0].shape[0] if stacked else len(ws)
    n, k = ws[0].shape[-2:]
    return (
        _use_hip(x, *ws)
        and x.dtype == torch.bfloat16
        and all(w.dtype == torch.bfloat16 for w in ws)
        and 1 <= n_exp <= GROUPED_MAX_EXPERTS
        and n % 128 == 0
        and k % 128 == 0
        and x.dim() == 2
        and x.shape[1] == k
    )


class _GroupedLinear(torch.autograd.Function):
    """The three grouped forms of gemm_tn8.  Weights stay separate tensors:
    the binding reads their base pointers, nothing is stacked per step, and
    wgrad's one [E,N,K] buffer is handed back as its slices."""

    @staticmethod
    def forward(ctx, x, offs, stacked, *ws):
        x = x.contiguous()
        ws = [w.contiguous() for w in ws]
        ctx.save_for_backward(x, offs, *ws)
        ctx.stacked = stacked
        return _ext().gemm_tn8(x, ws[0] if stacked else ws, 0, group_offsets=offs,
                               group_form="fwd")

    @staticmethod
    def backward(ctx, dy):
        x, offs, *ws = ctx.saved_tensors
        b = ws[0] if ctx.stacked else ws
        dy = dy.contiguous()
        dx = dws = None
        if ctx.needs_input_grad[0]:
            dx = _ext().gemm_tn8(dy, b, 0, group_offsets=offs, group_form="dgrad")
        if any(ctx.needs_input_grad[3:]):
            dw = _ext().gemm_tn8(dy, b, 0, group_offsets=offs, group_form="wgrad", group_x=x)
            dws = (dw,) if ctx.stacked else dw.unbind(0)
        else:
            dws = (None,) * len(ws)
        return (dx, None, None, *dws)


def grouped_linear(x: torch.Tensor, weights, group_offsets: torch.Tensor) -> torch.Tensor:
    """y[t] = x[t] @ weights[e(t)]^T for rows sorted by expert.

    x [T,K]; weights: E tensors [N,K] or one [E,N,K]; group_offsets [E+1]
    (int32 on the HIP path): expert e owns rows offs[e]..offs[e+1], offs[0] = 0
    and offs[E] = T.  bf16 on the GPU inside the shape contract
    (`grouped_fits`) is one HIP launch per GEMM, forward and backward, with
    no host sync; everything else is a per-group loop that reads the offsets
    on the host."""
    ws, stacked = _weight_list(weights)
    if grouped_fits(x, weights):
        offs = group_offsets.to(torch.int32).contiguous()
        return _GroupedLinear.apply(x, offs, stacked, *ws)
    bounds = group_offsets.tolist()
    mats = ws[0].unbind(0) if stacked else ws
    out = x.new_zeros(x.shape[0], mats[0].shape[0])
    for e, w in enumerate(mats):
        lo, hi = bounds[e], bounds[e + 1]
        if hi > lo:
            out[lo:hi] = torch.nn.functional.linear(x[lo:hi], w)
    return out
