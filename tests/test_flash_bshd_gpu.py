"""The [B,S,Hq,D] output layout of the tuned flash attention: fa_fwd(...,
out_bshd=True) and fa_bwd2(..., bshd=True) must be the default calls with o
and dout transposed, bitwise, and flash_attention_causal must hand the model
an output whose transpose(1, 2).reshape(B, S, H*D) is a view.

S = 768 gives 6 forward q tiles and 3 dq tiles per head (fa2_dq walks its
tiles heaviest first), so a wrong tile map shows as a wrong tile against
SDPA; S = 256 is the one-dq-tile edge."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

SHAPES = [(2, 4, 2, 768), (1, 2, 1, 256)]
D = 128


def _inputs(B, Hq, Hkv, S, seed):
    torch.manual_seed(seed)
    q = torch.randn(B, Hq, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
    dy = torch.randn(B, Hq, S, D, device="cuda", dtype=torch.bfloat16)
    return q, k, v, dy


def _sdpa_grads(q, k, v, dy):
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=True)
    ref.backward(dy)
    return q.grad, k.grad, v.grad


def _check_grads(got, want):
    for name, g, r, atol, rtol in zip(("dq", "dk", "dv"), got, want,
                                      (6e-2, 8e-2, 8e-2), (8e-2, 1e-1, 1e-1)):
        err = (g.float() - r.float()).abs().max().item()
        print(f"{name}: max abs err {err:.3e}")
        assert torch.allclose(g.float(), r.float(), atol=atol, rtol=rtol), (name, err)


@requires_gpu
@pytest.mark.parametrize("B,Hq,Hkv,S", SHAPES)
def test_fa_fwd_out_bshd(B, Hq, Hkv, S):
    import vescale_amd.ops as ops

    C = ops.require_ext()
    q, k, v, _ = _inputs(B, Hq, Hkv, S, 21)
    sc = 1.0 / math.sqrt(D)
    o, lse = C.fa_fwd(q, k, v, sc)
    o2, lse2 = C.fa_fwd(q, k, v, sc, out_bshd=True)
    assert o2.shape == (B, S, Hq, D) and o2.is_contiguous()
    assert lse2.shape == (B, Hq, S)
    assert torch.equal(o2, o.transpose(1, 2))
    assert torch.equal(lse2, lse)
    # test_flash_attention_fwd_kernel's reference and tolerance
    kx = k.float().repeat_interleave(Hq // Hkv, 1)
    vx = v.float().repeat_interleave(Hq // Hkv, 1)
    ref = F.scaled_dot_product_attention(q.float(), kx, vx, is_causal=True)
    err = (o2.transpose(1, 2).float() - ref).abs() / ref.abs().clamp_min(1.0)
    print(f"o: max err {err.max().item():.3e}")
    assert err.max().item() < 2e-2, err.max().item()
    s_full = torch.einsum("bhqd,bhkd->bhqk", q.float(), kx) * sc
    mask = torch.full((S, S), float("-inf"), device="cuda").triu(1)
    assert (lse2 - (s_full + mask).logsumexp(-1)).abs().max().item() < 1e-2


@requires_gpu
@pytest.mark.parametrize("B,Hq,Hkv,S", SHAPES)
def test_fa_bwd2_bshd(B, Hq, Hkv, S):
    import vescale_amd.ops as ops

    C = ops.require_ext()
    q, k, v, dy = _inputs(B, Hq, Hkv, S, 22)
    sc = 1.0 / math.sqrt(D)
    o, lse = C.fa_fwd(q, k, v, sc)
    base = C.fa_bwd2(q, k, v, o, dy, lse, sc, False)
    got = C.fa_bwd2(q, k, v, o.transpose(1, 2).contiguous(), dy.transpose(1, 2).contiguous(),
                    lse, sc, False, bshd=True)
    for name, g, b in zip(("dq", "dk", "dv"), got, base):
        assert g.shape == b.shape and g.is_contiguous(), name
        assert torch.equal(g, b), f"{name} differs between the layouts"
    _check_grads(got, _sdpa_grads(q, k, v, dy))


@requires_gpu
@pytest.mark.parametrize("B,Hq,Hkv,S", SHAPES)
def test_flash_attention_causal_no_copy(B, Hq, Hkv, S):
    from vescale_amd.ops import flash_attention_causal

    q, k, v, dy = _inputs(B, Hq, Hkv, S, 23)
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = flash_attention_causal(qq, kk, vv)
    assert o.shape == (B, Hq, S, D)
    flat = o.transpose(1, 2).reshape(B, S, -1)
    assert flat.data_ptr() == o.data_ptr() and flat.is_contiguous(), "reshape made a copy"
    # the model's path: the gradient arrives on the flattened view
    flat.backward(dy.transpose(1, 2).reshape(B, S, -1))
    _check_grads((qq.grad, kk.grad, vv.grad), _sdpa_grads(q, k, v, dy))
    # a caller that differentiates the [B,H,S,D] result directly gets the same
    q2, k2, v2 = (t.clone().requires_grad_(True) for t in (q, k, v))
    flash_attention_causal(q2, k2, v2).backward(dy)
    assert torch.equal(q2.grad, qq.grad) and torch.equal(k2.grad, kk.grad)
    assert torch.equal(v2.grad, vv.grad)
