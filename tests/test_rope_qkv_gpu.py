"""Fused qkv-split + RoPE kernels (rope_qkv.hip), both forms: the 16-byte
kernels (D % 16 == 0) and the scalar ones (any even D), against the fp32
torch path of _RoPEQKV run on CPU copies of the same bf16 inputs.

Every roped output is ONE bf16 rounding of an fp32 expression of two inputs,
so |out - ref| <= 2^-8 |ref| + 2^-22 (|x0| + |x1|), ref being that fp32
expression: half a bf16 ulp of the result plus the fp32 products and sum,
which the two paths may contract differently.  The reference therefore gets
the bf16 inputs widened to fp32 (exact), so that it returns the unrounded
value the bound is about.  V, and dv inside dqkv, are moved, never computed:
bitwise equal to their source."""
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

SHAPES = [(2, 5, 4, 2, 128), (1, 1, 1, 1, 128), (2, 7, 3, 1, 64), (1, 4, 2, 1, 8), (1, 3, 2, 2, 16)]


def _halves(t, D):
    """|x0| + |x1| per output element of a [..., D] tensor of rotation pairs."""
    a = t.float().abs()
    s = a[..., : D // 2] + a[..., D // 2:]
    return torch.cat([s, s], dim=-1)


def _check(out, ref, mag, what):
    out, ref = out.float().cpu(), ref.float()
    err = (out - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -22 * mag
    worst = float((err - bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, max (err - bound) {worst:.3e}")
    assert bool((err <= bound).all()), (what, worst)


@requires_gpu
@pytest.mark.parametrize("pos_offset", [0, 3])
@pytest.mark.parametrize("B,S,Hq,Hkv,D", SHAPES)
def test_rope_qkv_fwd_bwd(B, S, Hq, Hkv, D, pos_offset):
    from vescale_amd.ops import build_rope_table, rope_qkv

    torch.manual_seed(5)
    table = build_rope_table(S + pos_offset + 6, D)  # longer than S + pos_offset
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, dtype=torch.bfloat16)
    dq = torch.randn(B, Hq, S, D, dtype=torch.bfloat16)
    dk = torch.randn(B, Hkv, S, D, dtype=torch.bfloat16)
    dv = torch.randn(B, Hkv, S, D, dtype=torch.bfloat16)

    def run(dev, dtype):
        x = qkv.to(dev, dtype).requires_grad_(True)
        q, k, v = rope_qkv(x, table.to(dev), Hq, Hkv, D, pos_offset)
        torch.autograd.backward(
            [q, k, v], [dq.to(dev, dtype), dk.to(dev, dtype), dv.to(dev, dtype)])
        return q.detach(), k.detach(), v.detach(), x.grad

    q, k, v, g = run("cuda", torch.bfloat16)
    rq, rk, rv, rg = run("cpu", torch.float32)
    assert q.shape == (B, Hq, S, D) and k.shape == (B, Hkv, S, D) and v.shape == (B, Hkv, S, D)
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous()

    nq, nk = Hq * D, Hkv * D
    xq = qkv[..., :nq].reshape(B, S, Hq, D).transpose(1, 2)
    xk = qkv[..., nq:nq + nk].reshape(B, S, Hkv, D).transpose(1, 2)
    xv = qkv[..., nq + nk:].reshape(B, S, Hkv, D).transpose(1, 2)
    _check(q, rq, _halves(xq, D), "q")
    _check(k, rk, _halves(xk, D), "k")
    assert torch.equal(v.cpu(), xv), "v must be a bitwise copy"

    assert g.shape == qkv.shape
    g = g.cpu()
    _check(g[..., :nq], rg[..., :nq],
           _halves(dq, D).transpose(1, 2).reshape(B, S, nq), "dqkv[q]")
    _check(g[..., nq:nq + nk], rg[..., nq:nq + nk],
           _halves(dk, D).transpose(1, 2).reshape(B, S, nk), "dqkv[k]")
    assert torch.equal(g[..., nq + nk:], dv.transpose(1, 2).reshape(B, S, nk)), \
        "dv inside dqkv must be a bitwise copy"


def _misaligned(t):
    """A contiguous copy of t that starts 2 bytes into its storage: the binding
    sends tensors that are not 16-byte aligned to the scalar kernels."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


@requires_gpu
@pytest.mark.parametrize("B,S,Hq,Hkv,D", [(2, 5, 4, 2, 128), (2, 7, 3, 1, 64), (1, 3, 2, 2, 16)])
def test_rope_qkv_forms_agree_bitwise(B, S, Hq, Hkv, D):
    """The 16-byte kernels round exactly as the scalar kernels do (one product
    rounded, the other fused into the sum, the same one): the same call on a misaligned
    copy, which runs the scalar kernels, gives bitwise the same q, k, v and
    dqkv, so a model's results do not depend on which form ran."""
    import vescale_amd.ops as ops

    C = ops.require_ext()
    torch.manual_seed(6)
    table = ops.build_rope_table(S + 4, D, device="cuda")
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16)
    dq = torch.randn(B, Hq, S, D, device="cuda", dtype=torch.bfloat16)
    dk = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
    dv = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
    assert qkv.data_ptr() % 16 == 0 and dq.data_ptr() % 16 == 0
    fast = C.rope_qkv_fwd(qkv, table, B, S, Hq, Hkv, D, 1)
    slow = C.rope_qkv_fwd(_misaligned(qkv), table, B, S, Hq, Hkv, D, 1)
    for name, a, b in zip("qkv", fast, slow):
        assert torch.equal(a, b), f"{name}: the two forms differ"
    gfast = C.rope_qkv_bwd(dq, dk, dv, table, B, S, Hq, Hkv, D, 1)
    gslow = C.rope_qkv_bwd(_misaligned(dq), dk, dv, table, B, S, Hq, Hkv, D, 1)
    assert torch.equal(gfast, gslow), "dqkv: the two forms differ"
