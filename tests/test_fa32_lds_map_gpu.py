"""The 32x32 flash kernels on the bank-conflict-free LDS tile map
(csrc/fa32_lds_map.h): the tr probe returns exactly the transposed tile, and
fa_fwd / fa_bwd2 (split and fused) match an fp32 reference and repeat bitwise.

Shapes (B, Hq, Hkv, S), D = 128: the group ratio 4 is the benchmark's; S = 512
is the smallest size with fully unmasked off-diagonal tiles for all eight
waves of a backward block and two dq tiles; S = 256 is the one-tile edge.
Tolerances are those of the existing tests of these kernels
(tests/test_flash_bshd_gpu.py)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

SHAPES = [(1, 4, 1, 256), (1, 4, 1, 512)]
D = 128
_cache = {}


def _case(shape):
    """Inputs, fp32 reference (o, lse, dq, dk, dv) and one run of the kernels,
    computed once per shape and shared, unchanged, by the tests."""
    if shape in _cache:
        return _cache[shape]
    import vescale_amd.ops as ops

    C = ops.require_ext()
    B, Hq, Hkv, S = shape
    g = torch.Generator(device="cuda").manual_seed(31 + S)
    q, k, v, dy = (torch.randn(B, h, S, D, device="cuda", dtype=torch.bfloat16, generator=g)
                   for h in (Hq, Hkv, Hkv, Hq))
    sc = 1.0 / math.sqrt(D)
    # fp32 reference, dense masked softmax, GQA by expanding the kv heads
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    kx = kf.repeat_interleave(Hq // Hkv, 1)
    vx = vf.repeat_interleave(Hq // Hkv, 1)
    s = torch.einsum("bhqd,bhkd->bhqk", qf, kx) * sc
    s = s + torch.full((S, S), float("-inf"), device="cuda").triu(1)
    ref_lse = s.logsumexp(-1)
    ref_o = torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, -1), vx)
    ref_o.backward(dy.float())
    ref = (ref_o.detach(), ref_lse.detach(), qf.grad, kf.grad, vf.grad)

    o, lse = C.fa_fwd(q, k, v, sc)
    dq, dk, dv = C.fa_bwd2(q, k, v, o, dy, lse, sc, False)
    _cache[shape] = dict(C=C, q=q, k=k, v=v, dy=dy, sc=sc, ref=ref, got=(o, lse, dq, dk, dv))
    return _cache[shape]


def _check_fwd(o, lse, ref):
    err = ((o.float() - ref[0]).abs() / ref[0].abs().clamp_min(1.0)).max().item()
    lerr = (lse - ref[1]).abs().max().item()
    print(f"o: max err rel. to max(|ref|, 1) {err:.3e}; lse: max abs err {lerr:.3e}")
    assert err < 2e-2, err
    assert lerr < 1e-2, lerr


def _check_grads(got, want):
    for name, g, r, atol, rtol in zip(("dq", "dk", "dv"), got, want,
                                      (6e-2, 8e-2, 8e-2), (8e-2, 1e-1, 1e-1)):
        err = (g.float() - r).abs().max().item()
        print(f"{name}: max abs err {err:.3e}")
        assert torch.allclose(g.float(), r, atol=atol, rtol=rtol), (name, err)


@requires_gpu
def test_tr_probe_exact():
    """Every element the tr reads return is the transposed tile's:
    out[ds, ks, lane, e] = (ks*16 + half*8 + e)*128 + ds*32 + l31."""
    import vescale_amd.ops as ops

    out = ops.require_ext().tr_probe().cpu().to(torch.int64) & 0xFFFF
    assert out.shape == (4, 4, 64, 8)
    ds = torch.arange(4).view(4, 1, 1, 1)
    ks = torch.arange(4).view(1, 4, 1, 1)
    lane = torch.arange(64).view(1, 1, 64, 1)
    e = torch.arange(8).view(1, 1, 1, 8)
    want = (ks * 16 + (lane >> 5) * 8 + e) * 128 + ds * 32 + (lane & 31)
    bad = (out != want).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} of {want.numel()} differ, first {bad[:4].tolist()}"


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fwd_accuracy(shape):
    c = _case(shape)
    _check_fwd(c["got"][0], c["got"][1], c["ref"])


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bwd_accuracy(shape):
    c = _case(shape)
    _check_grads(c["got"][2:], c["ref"][2:])


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_run_to_run_bitwise(shape):
    """A second call on the same inputs gives the same bits (a wrong
    asynchronous-LDS-read pattern showed as run-to-run differences before)."""
    c = _case(shape)
    C = c["C"]
    o, lse = C.fa_fwd(c["q"], c["k"], c["v"], c["sc"])
    again = (o, lse) + tuple(C.fa_bwd2(c["q"], c["k"], c["v"], o, c["dy"], lse, c["sc"], False))
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), again, c["got"]):
        assert torch.equal(a, b), f"{name} differs between two calls"


@requires_gpu
def test_fused_dvdk_accuracy():
    """The kept-for-A/B fused dV+dK kernel reads the same tiles through the
    same helpers."""
    c = _case(SHAPES[0])
    o, lse = c["got"][:2]
    got = c["C"].fa_bwd2(c["q"], c["k"], c["v"], o, c["dy"], lse, c["sc"], True)
    _check_grads(got, c["ref"][2:])
