"""The per-tile paths of the 32x32 flash kernels (fa_fwd, fa2_dq / fa2_dk /
fa2_dv): a wave takes the unmasked path off the diagonal, the masked path on
it and no path at all above it, and the choice is made per tile and per wave.

- Against SDPA autograd at S = 256 (one backward block: its wave 7 alone sees
  unmasked, masked and inactive tiles), S = 512 (adds a block that starts off
  the diagonal) and S = 768 (adds fa2_dq's descending tile walk), in both
  layouts of o / dout; tolerances are those of test_flash_bshd_gpu.py.
- Causal independence, bitwise: what lies in a row's causal future must not
  reach it.  A tile that wrongly took the unmasked path mixes future rows in
  and shows here as a changed bit, where a tolerance against SDPA could still
  pass.  The cut points sit inside a wave's 32 rows (200, 300), on a wave
  boundary (32) and on a block boundary (256).
- The relayout probe: ff_relayout (two-operand permlane32_swap, no select)
  returns the bits of its earlier formulation (one-operand swap and two
  selects), kept in probes.hip for this comparison, and both are the
  B-operand fragment layout worked out on the host.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

D = 128
SHAPES = [(1, 2, 1, 256), (1, 4, 2, 512), (2, 4, 2, 768)]
SC = 1.0 / math.sqrt(D)


def _ext():
    import vescale_amd.ops as ops

    return ops.require_ext()


def _randn(gen, *shape):
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16, generator=gen)


@functools.lru_cache(maxsize=None)
def _case(B, Hq, Hkv, S):
    """Inputs and the SDPA reference of one shape, computed once and shared
    (read-only) by the tests of that shape."""
    gen = torch.Generator(device="cuda").manual_seed(1000 + S)
    q, dy = _randn(gen, B, Hq, S, D), _randn(gen, B, Hq, S, D)
    k, v = _randn(gen, B, Hkv, S, D), _randn(gen, B, Hkv, S, D)
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qr, kr, vr, is_causal=True, enable_gqa=True)
    ref.backward(dy)
    kx = k.float().repeat_interleave(Hq // Hkv, 1)
    vx = v.float().repeat_interleave(Hq // Hkv, 1)
    o32 = F.scaled_dot_product_attention(q.float(), kx, vx, is_causal=True)
    s_full = torch.einsum("bhqd,bhkd->bhqk", q.float(), kx) * SC
    mask = torch.full((S, S), float("-inf"), device="cuda").triu(1)
    lse32 = (s_full + mask).logsumexp(-1)
    return q, k, v, dy, o32, lse32, (qr.grad, kr.grad, vr.grad)


@requires_gpu
@pytest.mark.parametrize("bshd", [False, True])
@pytest.mark.parametrize("B,Hq,Hkv,S", SHAPES)
def test_split_path_vs_sdpa(B, Hq, Hkv, S, bshd):
    C = _ext()
    q, k, v, dy, o32, lse32, grads = _case(B, Hq, Hkv, S)
    o, lse = C.fa_fwd(q, k, v, SC, out_bshd=bshd)
    o_bhsd = o.transpose(1, 2) if bshd else o
    err = (o_bhsd.float() - o32).abs() / o32.abs().clamp_min(1.0)
    print(f"o: max err {err.max().item():.3e}")
    assert err.max().item() < 2e-2, err.max().item()
    lerr = (lse - lse32).abs().max().item()
    print(f"lse: max abs err {lerr:.3e}")
    assert lerr < 1e-2, lerr
    dout = dy.transpose(1, 2).contiguous() if bshd else dy
    got = C.fa_bwd2(q, k, v, o, dout, lse, SC, False, bshd=bshd)
    for name, g, r, atol, rtol in zip(("dq", "dk", "dv"), got, grads,
                                      (6e-2, 8e-2, 8e-2), (8e-2, 1e-1, 1e-1)):
        gerr = (g.float() - r.float()).abs().max().item()
        print(f"{name}: max abs err {gerr:.3e}")
        assert torch.allclose(g.float(), r.float(), atol=atol, rtol=rtol), (name, gerr)


CUT_S = 512
CUT_SHAPE = (1, 4, 2, CUT_S)


def _rows(t, lo, hi, bshd=False):
    """Rows lo..hi of the sequence axis of a [B,H,S,*] (or, bshd, [B,S,H,*]) tensor."""
    return t[:, lo:hi] if bshd else t[:, :, lo:hi]


@requires_gpu
@pytest.mark.parametrize("bshd", [False, True])
@pytest.mark.parametrize("p", [32, 200, 256, 300])
def test_rows_before_cut_ignore_later_kv(p, bshd):
    """K and V rows >= p replaced: O, lse and dQ rows < p keep every bit."""
    C = _ext()
    q, k, v, dy = _case(*CUT_SHAPE)[:4]
    dout = dy.transpose(1, 2).contiguous() if bshd else dy
    o, lse = C.fa_fwd(q, k, v, SC, out_bshd=bshd)
    dq = C.fa_bwd2(q, k, v, o, dout, lse, SC, False, bshd=bshd)[0]

    gen = torch.Generator(device="cuda").manual_seed(7 + p)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, p:] = _randn(gen, *k[:, :, p:].shape)
    v2[:, :, p:] = _randn(gen, *v[:, :, p:].shape)
    o2, lse2 = C.fa_fwd(q, k2, v2, SC, out_bshd=bshd)
    assert not torch.equal(_rows(o2, p, CUT_S, bshd), _rows(o, p, CUT_S, bshd)), "nothing was perturbed"
    assert torch.equal(_rows(o2, 0, p, bshd), _rows(o, 0, p, bshd)), "o rows < p changed"
    assert torch.equal(lse2[:, :, :p], lse[:, :, :p]), "lse rows < p changed"
    # rows < p of the backward's o and lse are the unperturbed forward's
    o2 = o2.clone()
    lse2 = lse2.clone()
    _rows(o2, 0, p, bshd).copy_(_rows(o, 0, p, bshd))
    lse2[:, :, :p] = lse[:, :, :p]
    dq2 = C.fa_bwd2(q, k2, v2, o2, dout, lse2, SC, False, bshd=bshd)[0]
    assert torch.equal(dq2[:, :, :p], dq[:, :, :p]), "dq rows < p changed"


@requires_gpu
@pytest.mark.parametrize("bshd", [False, True])
@pytest.mark.parametrize("p", [32, 200, 256, 300])
def test_rows_from_cut_ignore_earlier_q(p, bshd):
    """Q and dO rows < p replaced: dK and dV rows >= p keep every bit."""
    C = _ext()
    q, k, v, dy = _case(*CUT_SHAPE)[:4]
    dout = dy.transpose(1, 2).contiguous() if bshd else dy
    o, lse = C.fa_fwd(q, k, v, SC, out_bshd=bshd)
    _, dk, dv = C.fa_bwd2(q, k, v, o, dout, lse, SC, False, bshd=bshd)

    gen = torch.Generator(device="cuda").manual_seed(11 + p)
    q2, dout2 = q.clone(), dout.clone()
    q2[:, :, :p] = _randn(gen, *q[:, :, :p].shape)
    _rows(dout2, 0, p, bshd).copy_(_randn(gen, *_rows(dout, 0, p, bshd).shape))
    o2, lse2 = C.fa_fwd(q2, k, v, SC, out_bshd=bshd)
    assert torch.equal(_rows(o2, p, CUT_S, bshd), _rows(o, p, CUT_S, bshd)), "o rows >= p changed"
    assert torch.equal(lse2[:, :, p:], lse[:, :, p:]), "lse rows >= p changed"
    # rows >= p of the backward's o and lse are the unperturbed forward's
    o2 = o2.clone()
    lse2 = lse2.clone()
    _rows(o2, p, CUT_S, bshd).copy_(_rows(o, p, CUT_S, bshd))
    lse2[:, :, p:] = lse[:, :, p:]
    _, dk2, dv2 = C.fa_bwd2(q2, k, v, o2, dout2, lse2, SC, False, bshd=bshd)
    assert not torch.equal(dk2[:, :, :p], dk[:, :, :p]), "nothing was perturbed"
    assert torch.equal(dk2[:, :, p:], dk[:, :, p:]), "dk rows >= p changed"
    assert torch.equal(dv2[:, :, p:], dv[:, :, p:]), "dv rows >= p changed"


def _probe_inputs(kind):
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(64, 32, device="cuda", generator=gen)
    if kind == "special":
        # +-inf, +-0, fp32 denormals, values that round to bf16 denormals and
        # the largest finite values, scattered over lanes and registers
        specials = torch.tensor(
            [float("inf"), float("-inf"), 0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1e-39, -3e-39,
             1.17549435e-38, 3.3e38, -3.4028235e38], device="cuda")
        idx = torch.randint(0, specials.numel() + 4, (64, 32), device="cuda", generator=gen)
        x = torch.where(idx < specials.numel(), specials[idx.clamp_max(specials.numel() - 1)], x)
    return x


@requires_gpu
@pytest.mark.parametrize("kind", ["random", "special"])
def test_relayout_probe_matches_earlier_formulation(kind):
    C = _ext()
    x = _probe_inputs(kind)
    out = C._relayout_probe(x)
    assert out.shape == (2, 64, 4, 8) and out.dtype == torch.int16
    assert torch.equal(out[1], out[0]), "ff_relayout differs from its earlier formulation"


@requires_gpu
def test_relayout_probe_is_the_b_fragment_layout():
    """Fragment f = s2*2 + g of lane (l31, half) holds rows g*16 + half*8 + e
    (e = 0..7) of subtile s2, column l31; D-layout register r of half h holds
    row (r & 3) + 8 * (r >> 2) + 4 * h."""
    C = _ext()
    x = _probe_inputs("random")
    got = C._relayout_probe(x)[1].view(torch.bfloat16).cpu()
    xb = x.to(torch.bfloat16).cpu()  # round to nearest even, as v_cvt_pk_bf16_f32
    want = torch.empty(64, 4, 8, dtype=torch.bfloat16)
    for lane in range(64):
        l31, half = lane & 31, lane >> 5
        for s2 in range(2):
            for g in range(2):
                for e in range(8):
                    rr = g * 16 + half * 8 + e
                    r = (rr & 3) + 4 * (rr >> 3)
                    src = l31 + 32 * ((rr >> 2) & 1)
                    want[lane, s2 * 2 + g, e] = xb[src, s2 * 16 + r]
    assert torch.equal(got, want)
