"""Direct global -> LDS staging of the tuned 32x32 flash kernels (ff_stage_async,
csrc/fa32_common.h) on the GPU.

1. The staging probe: one tile staged by ff_stage_rows and by ff_stage_async
   into two LDS arrays; the two images are bitwise equal and are the image of
   fa32_lds_map.h worked out on the host.
2. fa_fwd / fa_bwd2 against SDPA with the tolerances of test_flash_bshd_gpu.py,
   in both layouts.  S = 256 is 4 kv tiles in one block (both buffers, the
   wrap-around), S = 512 adds blocks with different trip counts, S = 768
   fa2_dq's descending walk; the packed-document case (documents starting at
   64 and 192) makes a block's first tile odd, so a stale buffer or a parity
   slip shows.
3. Races: five calls on the same inputs give the same bits, and those bits are
   the ones recorded from the build before the direct staging
   (tests/golden/fa32_parent_digests.json).  Inputs come from a seeded CPU
   generator, so they do not depend on the device RNG.
"""
import functools
import hashlib
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")]

D = 128
SCALE = 1.0 / math.sqrt(D)
SEG_LENGTHS = (64, 128, 320)  # documents start at 0, 64 and 192
# name: (B, Hq, Hkv, S, bshd, packed documents)
CASES = {}
for _shape in ((1, 2, 1, 256), (1, 4, 2, 512), (2, 4, 2, 768)):
    for _bshd in (False, True):
        CASES["-".join(map(str, _shape)) + ("-bshd" if _bshd else "-bhsd")] = (*_shape, _bshd, False)
for _bshd in (False, True):
    CASES["1-4-2-512-seg" + ("-bshd" if _bshd else "-bhsd")] = (1, 4, 2, 512, _bshd, True)
NAMES = ("o", "lse", "dq", "dk", "dv")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "fa32_parent_digests.json")


def make_inputs(name):
    """q, k, v [B,H,S,D], dout in the case's layout, segment ids or None; bf16 on
    the device, drawn on the CPU."""
    B, Hq, Hkv, S, bshd, seg = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    q, dout = (torch.randn(B, Hq, S, D, generator=g).bfloat16() for _ in range(2))
    k, v = (torch.randn(B, Hkv, S, D, generator=g).bfloat16() for _ in range(2))
    if bshd:
        dout = dout.transpose(1, 2).contiguous()
    ids = None
    if seg:
        row = torch.cat([torch.full((n,), i, dtype=torch.int32)
                         for i, n in enumerate(SEG_LENGTHS)])
        assert row.numel() == S
        ids = row.expand(B, S).contiguous().cuda()
    return q.cuda(), k.cuda(), v.cuda(), dout.cuda(), ids


def run_kernels(name, inputs):
    """One fwd + bwd through the bindings: (o, lse, dq, dk, dv), o in the case's layout."""
    import vescale_amd.ops as ops
    C = ops.require_ext()
    bshd = CASES[name][4]
    q, k, v, dout, ids = inputs
    if ids is None:
        o, lse = C.fa_fwd(q, k, v, SCALE, out_bshd=bshd)
        bounds = None
    else:
        o, lse, bounds = C.fa_fwd(q, k, v, SCALE, out_bshd=bshd, segment_ids=ids)
    dq, dk, dv = C.fa_bwd2(q, k, v, o, dout, lse, SCALE, False, bshd=bshd, seg_bounds=bounds)
    return o, lse, dq, dk, dv


def digests(outs):
    torch.cuda.synchronize()
    return {n: hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
            for n, t in zip(NAMES, outs)}


@functools.lru_cache(maxsize=None)
def _results(name):
    inputs = make_inputs(name)
    return inputs, [run_kernels(name, inputs) for _ in range(5)]


def _reference(name, inputs):
    """SDPA: o and lse in fp32; gradients as test_flash_bshd_gpu.py takes them
    (bf16, enable_gqa), with packed documents in fp32 under an explicit mask."""
    B, Hq, Hkv, S, bshd, seg = CASES[name]
    q, k, v, dout, ids = inputs
    dy = dout.transpose(1, 2) if bshd else dout
    vis = torch.ones(S, S, dtype=torch.bool, device="cuda").tril()
    if seg:
        vis = vis & (ids[0][:, None] == ids[0][None, :])
    kx = k.float().repeat_interleave(Hq // Hkv, 1)
    vx = v.float().repeat_interleave(Hq // Hkv, 1)
    o = F.scaled_dot_product_attention(q.float(), kx, vx, attn_mask=vis)
    s_full = torch.einsum("bhqd,bhkd->bhqk", q.float(), kx) * SCALE
    lse = s_full.masked_fill(~vis, float("-inf")).logsumexp(-1)
    if seg:
        qq, kk, vv = (t.float().detach().clone().requires_grad_(True) for t in (q, k, v))
        g = Hq // Hkv
        F.scaled_dot_product_attention(qq, kk.repeat_interleave(g, 1), vv.repeat_interleave(g, 1),
                                       attn_mask=vis).backward(dy.float())
    else:
        qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        F.scaled_dot_product_attention(qq, kk, vv, is_causal=True, enable_gqa=True).backward(dy)
    return o, lse, qq.grad, kk.grad, vv.grad


@pytest.mark.parametrize("rows,threads,stride", [
    (64, 256, 128), (64, 512, 128), (256, 512, 128),
    (64, 256, 4 * 128), (64, 512, 4 * 128), (256, 512, 4 * 128), (256, 512, 32 * 128),
])
def test_stage_probe_images_are_equal(rows, threads, stride):
    import vescale_amd.ops as ops
    C = ops.require_ext()
    g = torch.Generator().manual_seed(rows + threads + stride)
    # distinct 16-bit patterns per element, every bit pattern class included
    x = torch.randint(-2 ** 15, 2 ** 15, (rows, stride), generator=g, dtype=torch.int16)
    out = C._stage_probe(x.view(torch.bfloat16).cuda(), threads).cpu()
    assert out.shape == (2, rows, D)
    assert torch.equal(out[0], out[1]), "direct staging differs from ff_stage_rows"
    # the image itself: 16-byte slot s of row r holds slot s ^ g(r) of the tile row
    r = torch.arange(rows)
    gr = ((r & 3) << 2) | ((r >> 2) & 3)
    src = (torch.arange(16)[None, :] ^ gr[:, None])  # [rows, 16]
    want = x[:, :D].reshape(rows, 16, 8).gather(1, src[:, :, None].expand(rows, 16, 8))
    assert torch.equal(out[1], want.reshape(rows, D))


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_sdpa(name):
    B, Hq, Hkv, S, bshd, seg = CASES[name]
    inputs, runs = _results(name)
    o, lse, dq, dk, dv = runs[0]
    ro, rlse, rdq, rdk, rdv = _reference(name, inputs)
    if bshd:
        assert o.shape == (B, S, Hq, D)
        o = o.transpose(1, 2)
    err = ((o.float() - ro).abs() / ro.abs().clamp_min(1.0)).max().item()
    lerr = (lse - rlse).abs().max().item()
    print(f"o: max err {err:.3e}  lse: max abs err {lerr:.3e}")
    assert err < 2e-2, err
    assert lerr < 1e-2, lerr
    for nm, g, r, atol, rtol in zip(("dq", "dk", "dv"), (dq, dk, dv), (rdq, rdk, rdv),
                                    (6e-2, 8e-2, 8e-2), (8e-2, 1e-1, 1e-1)):
        gerr = (g.float() - r.float()).abs().max().item()
        print(f"{nm}: max abs err {gerr:.3e}")
        assert torch.allclose(g.float(), r.float(), atol=atol, rtol=rtol), (nm, gerr)


@pytest.mark.parametrize("name", sorted(CASES))
def test_five_calls_give_the_recorded_bits(name):
    _, runs = _results(name)
    for i, again in enumerate(runs[1:], 1):
        for nm, a, b in zip(NAMES, runs[0], again):
            assert torch.equal(a, b), f"{nm} of call {i} differs from call 0"
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = digests(runs[0])
    print(got)
    assert got == golden["digests"][name], f"bits differ from build {golden['parent_commit']}"
