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
    """gu = [.., 2F] (gate||up) -> [.., F]; avoids split+cat round trips."""

    @staticmethod
    def forward(ctx, gu: torch.Tensor):
        if _use_hip(gu):
            g = gu.contiguous()
            ctx.save_for_backward(g)
            ctx.hip = True
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
            return _ext().swiglu_packed_bwd(dy.contiguous(), gu)
        F = gu.shape[-1] // 2
        g = gu[..., :F].float()
        u = gu[..., F:].float()
        d = dy.float()
        sig = torch.sigmoid(g)
        dgate = d * u * sig * (1 + g * (1 - sig))
        dup = _swiglu_dup(d, g, sig)
        return torch.cat([dgate, dup], dim=-1).to(gu.dtype)


def swiglu_packed(gu: torch.Tensor) -> torch.Tensor:
    return _SwiGLUPacked.apply(gu)


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
# head_dim 128, GQA, seq % 256 == 0.
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
    def forward(ctx, q, k, v, scale):
        # q,k,v: [B, H, S, D] contiguous bf16.  The kernel writes o as
        # [B, S, H, D], the layout the output projection reads; callers get
        # the [B, H, S, D]-shaped view of it.
        out, lse = _ext().fa_fwd(q, k, v, scale, out_bshd=True)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.scale = scale
        return out.transpose(1, 2)

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
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
            return dq, dk, dv, None
        # the gradient of the [B, H, S, D] view of a [B, S, H*D] consumer is
        # contiguous once transposed back: no copy on the model's path
        dout = dout.transpose(1, 2)
        if not dout.is_contiguous():
            dout = dout.contiguous()
        dq, dk, dv = _ext().fa_bwd2(q, k, v, out, dout, lse, ctx.scale, False, bshd=True)
        return dq, dk, dv, None


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
                   kv_seg=None):
    """Differentiable torch attention returning (out, lse): the CPU path and
    the oracle of the general kernel.  Matmuls and softmax run in `dtype`
    (default: fp32, or q's dtype if wider); GQA by head grouping; key j is
    visible to query i iff j <= i + shift and, with q_seg [B,Sq] / kv_seg
    [B,Sk] given, kv_seg[b, j] == q_seg[b, i]; a row with no visible key
    gives out = 0, lse = -inf and zero gradients."""
    if dtype is None:
        dtype = torch.promote_types(q.dtype, torch.float32)
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    qg = q.to(dtype).reshape(B, Hkv, Hq // Hkv, Sq, D)
    s = (qg @ k.to(dtype).unsqueeze(2).transpose(-1, -2)) * scale
    if is_causal:
        i = torch.arange(Sq, device=q.device).unsqueeze(1)
        j = torch.arange(Sk, device=q.device).unsqueeze(0)
        s = s.masked_fill(j > i + shift, float("-inf"))
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
    fa_gen_bwd, which derives its tile bounds again."""

    @staticmethod
    def forward(ctx, q, k, v, scale, causal, shift, q_seg=None, kv_seg=None):
        out, lse = _ext().fa_gen_fwd(q, k, v, scale, causal, shift,
                                     q_seg=q_seg, kv_seg=kv_seg)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.args = (scale, causal, shift)
        ctx.seg = (q_seg, kv_seg)
        ctx.set_materialize_grads(False)
        return out, lse

    @staticmethod
    def backward(ctx, dout, dlse):
        q, k, v, out, lse = ctx.saved_tensors
        scale, causal, shift = ctx.args
        q_seg, kv_seg = ctx.seg
        dout = torch.zeros_like(out) if dout is None else dout.contiguous()
        if dlse is not None:
            dlse = dlse.float().contiguous()
        dq, dk, dv = _ext().fa_gen_bwd(
            q, k, v, out, dout, lse, dlse, scale, causal, shift,
            q_seg=q_seg, kv_seg=kv_seg
        )
        return dq, dk, dv, None, None, None, None, None


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


def flash_attention(q, k, v, *, is_causal=False, causal_shift=0, scale=None,
                    return_lse=False, q_segment_ids=None, kv_segment_ids=None):
    """Attention over q [B,Hq,Sq,D], k/v [B,Hkv,Sk,D] (Hq % Hkv == 0).

    With is_causal, key j is visible to query i iff j <= i + causal_shift
    (0: top-left triangle; Sk - Sq: bottom-right alignment).  A query row
    with no visible key yields out = 0, lse = -inf and zero gradients.
    Returns out, or (out, lse) with lse [B,Hq,Sq] fp32 (natural log) when
    return_lse; both outputs are differentiable.

    Packed sequences: with q_segment_ids [B,Sq] and kv_segment_ids [B,Sk]
    (any integer dtype) key j is visible to query i iff, in addition,
    kv_segment_ids[b, j] == q_segment_ids[b, i].  Ids are compared for
    equality only: no value is special and they need not be sorted.
    kv_segment_ids may be left out when Sq == Sk (the same ids for both);
    otherwise both are required (ValueError).  A query whose id no visible
    key carries is a dead row as above; a key no query sees gets zero dk/dv.
    segment_ids_from_cu_seqlens builds ids from document boundaries.

    Dispatch: (1) the tuned D=128 causal kernels when their gate holds, no
    lse is wanted and there are no segment ids; (2) the general HIP kernel
    for bf16 on GPU with D in {64, 128}; (3) the torch reference (CPU, other
    dtypes / head dims, VESCALE_FA=aten)."""
    import math

    if causal_shift != 0 and not is_causal:
        raise ValueError("causal_shift != 0 requires is_causal=True")
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
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
    if (hip and not return_lse and is_causal and causal_shift == 0
            and Sq == Sk and D == 128 and Sq % 256 == 0 and q_seg is None):
        return _FlashAttention.apply(
            q.contiguous(), k.contiguous(), v.contiguous(), scale
        )
    if hip:
        out, lse = _FlashAttentionGen.apply(
            q.contiguous(), k.contiguous(), v.contiguous(), float(scale),
            bool(is_causal), int(causal_shift),
            q_seg, kv_seg,
        )
    else:
        out, lse = _attention_ref(q, k, v, is_causal, causal_shift, scale,
                                  q_seg=q_seg, kv_seg=kv_seg)
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
#   "blaslt" (default) — torch.matmul -> hipBLASLt Tensile assembly kernels.
#   "gemm8"            — the in-tree 256x256 8-phase MFMA kernel
#                        (ops/csrc/gemm8.hip, rot3np schedule) for the
#                        forward and dgrad GEMMs; wgrad (both operands
#                        contraction-major) stays on the library until the
#                        tr-read wgrad kernel lands.  Honest A/B:
#                        profiles/gemm8_variants_ab_r2.log — the in-tree
#                        kernel is ~75% of hipBLASLt on Llama shapes, so
#                        blaslt remains the default (VERDICT r1 item 1:
#                        "do not ship a regression").
# Reference parity: sharded matmul family, SURVEY.md §2.7;
# legacy/vescale/dtensor/ops/matrix_ops.py:113.
def _gemm_backend() -> str:
    return os.environ.get("VESCALE_GEMM", "blaslt")


def _g8_ok(m: int, n: int, k: int) -> bool:
    return m % 256 == 0 and n % 256 == 0 and k % 64 == 0


class _Linear8(torch.autograd.Function):
    """y = x @ w^T via the in-tree TN kernel; dgrad = gemm_tn(dy, w^T)
    (one cheap [N,K]->[K,N] transpose per backward — arithmetic intensity
    of the GEMM is ~4 orders above the copy); wgrad on the library."""

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
            dw = dys.t() @ x2  # library wgrad (see header note)
        return dx, dw


def linear(x: torch.Tensor, w: torch.Tensor,
           bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    if _gemm_backend() == "gemm8" and bias is None:
        return _Linear8.apply(x, w)
    return torch.nn.functional.linear(x, w, bias)
