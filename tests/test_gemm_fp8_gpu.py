"""The fp8 GEMM, its quantiser kernels (csrc/gemm_fp8.hip, reached through
gemm_tn8) and linear() under VESCALE_GEMM=fp8.

Exact cases: operands k * 2^e with k in -4..4 (gemm_cases.exact_case, rows of a
scaled by 1, 2, 4 and rows of b by 1, 1/2) are e4m3 and e5m2 numbers, and every
product and partial sum is a multiple of 1/2 below 2^24 of them, exact in fp32
in any order: the result must be the bf16 rounding of the fp64 product.
Rounding cases: |err| <= 2^-8 |ref| + Kc 2^-23 (|A| @ |B|^T) scale_a scale_b, one
bf16 rounding plus a first-order fp32 accumulation bound over the contraction
length Kc (gemm_cases.rounding_bound, scaled)."""
import functools

import pytest
import torch

from tests import gemm_cases as gc

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")]

E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
FMAX = {E4M3: 448.0, E5M2: 57344.0}
DEPTH = 2  # K-tiles in flight: the prologue drains tile 0 and issues tile 1
# (M, N, K): one K tile, the depth boundaries, a 2 x 3 grid, a filled machine
EXACT_SHAPES = [(256, 256, 128 * n) for n in sorted({1, DEPTH - 1, DEPTH, DEPTH + 1, 5})]
EXACT_SHAPES += [(512, 768, 384), (4096, 4096, 256)]


def _ext():
    import vescale_amd.ops as ops

    return ops.require_ext()


def _s(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


@functools.lru_cache(maxsize=None)
def _exact(M, N, K):
    a, b = gc.exact_case(M, N, K)
    a = a.float() * (2.0 ** (torch.arange(M) % 3))[:, None]
    b = b.float() * (2.0 ** -(torch.arange(N) % 2))[:, None]
    return a, b, gc.product64(a, b)


@pytest.mark.parametrize("afmt", [E4M3, E5M2], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact(shape, afmt):
    a, b, ref = _exact(*shape)
    aq, bq = a.to(afmt), b.to(E4M3)
    assert torch.equal(aq.float(), a) and torch.equal(bq.float(), b)
    for sa, sb in ((1.0, 1.0), (0.5, 4.0)):
        got = _ext().gemm_tn8(aq.cuda(), bq.cuda(), 0, scale_a=_s(sa), scale_b=_s(sb)).cpu()
        want = (ref * (sa * sb)).float().bfloat16()
        bad = (got != want) | got.isnan()
        assert got.dtype == torch.bfloat16 and not bad.any(), (
            f"scales {sa, sb}: {int(bad.sum())} differ, first at {bad.nonzero()[0].tolist()}")


def _within_bound(got, aq64, bq64, s, tag):
    """got ~ (aq64 @ bq64^T) * s under the module's bound."""
    ref, bound = gc.rounding_bound(aq64, bq64)
    err = (got.cpu().double() - ref * s).abs()
    worst = (err / (bound * s).clamp_min(1e-300)).max().item()
    print(f"{tag}: max |err| / bound = {worst:.3f}")
    assert bool((err <= bound * s).all()), (tag, worst)


@pytest.mark.parametrize("afmt", [E4M3, E5M2], ids=["e4m3", "e5m2"])
def test_random(afmt):
    gen = torch.Generator().manual_seed(811)
    aq = torch.randn(512, 1024, generator=gen).to(afmt)
    bq = torch.randn(256, 1024, generator=gen).to(E4M3)
    sa, sb = 0.37, 1.9
    got = _ext().gemm_tn8(aq.cuda(), bq.cuda(), 0, scale_a=_s(sa), scale_b=_s(sb))
    s = float(torch.tensor(sa).float()) * float(torch.tensor(sb).float())
    _within_bound(got, aq.double(), bq.double(), s, f"random {afmt}")


def _quant_input(R, C, dtype, scale):
    """Gaussians around a block of edge values (times scale): zeros, exact ties
    between neighbouring fp8 numbers, values past +-fmt_max, values under half
    the smallest subnormal, and the smallest subnormal's own tie."""
    gen = torch.Generator().manual_seed(R * 1000 + C)
    x = torch.randn(R, C, generator=gen) * 3
    tiny = 2.0 ** (-9 if dtype == E4M3 else -16)  # smallest subnormal
    edge = [0.0, -0.0, 1.0625, 1.1875, -1.0625, 1.125, 1.375, 2.5, 3.5, FMAX[dtype],
            -FMAX[dtype], FMAX[dtype] * 1.06, -FMAX[dtype] * 1.5, 1e5, -3e38, tiny, tiny / 2,
            -tiny / 2, tiny * 1.5, tiny / 4, -tiny / 4, tiny * 0.75]
    x.view(-1)[:len(edge)] = torch.tensor(edge) * scale
    x[-1, -3:] = torch.tensor([FMAX[dtype] * 2, -tiny / 2, 0.0]) * scale
    return x.bfloat16()


@pytest.mark.parametrize("scale", [1.0, 0.25, 0.3])
@pytest.mark.parametrize("dtype", [E4M3, E5M2], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("shape", [(64, 64), (64, 192), (320, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantize(shape, dtype, scale):
    C = _ext()
    R, Cc = shape
    x = _quant_input(R, Cc, dtype, scale)
    sc = torch.tensor([scale], dtype=torch.float32)
    want = (x.float() / sc).clamp(-FMAX[dtype], FMAX[dtype]).to(dtype).view(torch.uint8)
    xd = x.cuda()
    amax = C.gemm_tn8(xd, [], 0, group_form="fp8_amax")
    assert amax.dtype == torch.float32 and amax.shape == (1,)
    assert amax.cpu().item() == x.abs().max().float().item()
    q = torch.empty(R, Cc, dtype=dtype, device="cuda")
    qt = torch.empty(Cc, R, dtype=dtype, device="cuda")
    out = C.gemm_tn8(xd, [], 0, group_form="fp8_quantize", scale_a=sc.cuda(), group_out=q, out_t=qt)
    assert out.data_ptr() == q.data_ptr()
    assert torch.equal(q.cpu().view(torch.uint8), want)
    assert torch.equal(qt.cpu().view(torch.uint8), want.t())
    # each output alone
    only_t = C.gemm_tn8(xd, [], 0, group_form="fp8_quantize", scale_a=sc.cuda(),
                        out_t=torch.empty_like(qt))
    assert torch.equal(only_t.cpu().view(torch.uint8), want.t())


def _quantized(t, dtype):
    """The CPU emulation of _fp8_quantize: (q as fp64, scale as fp32 [1])."""
    scale = (t.abs().max().float().reshape(1) / torch.tensor([FMAX[dtype]])).clamp_min(
        torch.finfo(torch.float32).tiny)
    return (t.float() / scale).clamp(-FMAX[dtype], FMAX[dtype]).to(dtype).double(), scale


def test_linear(monkeypatch):
    import vescale_amd.ops as ops

    monkeypatch.setenv("VESCALE_GEMM", "fp8")
    gen = torch.Generator().manual_seed(99)
    x = torch.randn(2, 256, 256, generator=gen).bfloat16()
    w = (torch.randn(768, 256, generator=gen) / 16).bfloat16()
    dy = torch.randn(2, 256, 768, generator=gen).bfloat16()
    xd, wd = x.cuda().requires_grad_(), w.cuda().requires_grad_()
    y = ops.linear(xd, wd)
    saved = y.grad_fn.saved_tensors
    assert y.shape == (2, 256, 768) and y.dtype == torch.bfloat16
    assert sorted(str(t.dtype) for t in saved) == sorted(
        ["torch.float8_e4m3fn"] * 2 + ["torch.float32"] * 2), [t.dtype for t in saved]
    y.backward(dy.cuda())

    (xq, sx), (wq, sw) = _quantized(x.reshape(-1, 256), E4M3), _quantized(w, E4M3)
    dyq, sd = _quantized(dy.reshape(-1, 768), E5M2)
    assert {float(t) for t in saved if t.dtype == torch.float32} == {float(sx), float(sw)}
    _within_bound(y.reshape(-1, 768), xq, wq, float(sx) * float(sw), "y")
    _within_bound(xd.grad.reshape(-1, 256), dyq, wq.t(), float(sd) * float(sw), "dx")
    _within_bound(wd.grad, dyq.t(), xq.t(), float(sd) * float(sx), "dw")


def test_linear_falls_back_outside_the_contract(monkeypatch):
    import vescale_amd.ops as ops

    monkeypatch.setenv("VESCALE_GEMM", "fp8")
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(512, 192, generator=gen).bfloat16().cuda()
    w = torch.randn(768, 192, generator=gen).bfloat16().cuda()
    assert torch.equal(ops.linear(x, w), torch.nn.functional.linear(x, w))
