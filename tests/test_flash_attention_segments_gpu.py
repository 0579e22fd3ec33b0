"""Segment-masked (packed-document) form of the general flash attention
kernels (ops/csrc/attention_gen.hip, SEG instantiations) on the GPU, by the
method of test_flash_attention_general_gpu.py: NaN arena, random dout and
dlse, and the same accuracy bound for every tensor x of o, dq, dk, dv:

    max|x - x32| <= 2 * max|x16 - x32| + 2^-8 * max|x32|

with x32 / x16 the torch reference given the same segment ids in fp32 / bf16,
and lse within 1e-2 on live rows.
"""
import functools
import math

import pytest
import torch

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

B = 2
PAD_ROWS = 64  # NaN rows on each side of every arena slice
NAN_BITS = torch.tensor(float("nan"), dtype=torch.bfloat16).view(torch.int16).item()


def _docs(*lengths, first=0):
    """ids of consecutive documents of the given lengths."""
    return torch.cat([torch.full((n,), first + d, dtype=torch.int32)
                      for d, n in enumerate(lengths)])


def _p5_q():
    ids = torch.zeros(64, dtype=torch.int32)
    ids[20:25] = 7          # carried by no key
    return ids


# name: (Sq, Sk, Hq, Hkv, causal, shift, q ids [Sq], kv ids [Sk] or None = q's)
CASES = {
    # an edge on (64 | 66) and off (1, 64+2) a tile boundary
    "p1": (130, 130, 4, 2, True, 0, _docs(1, 63, 2, 64), None),
    # tile pairs (0, 3) and (3, 0) skippable
    "p2": (200, 200, 4, 2, False, 0, _docs(70, 130), None),
    # cross shapes, different id tensors
    "p3": (70, 200, 4, 2, True, 130, _docs(20, 50), _docs(150, 50)),
    # unsorted: the skip test must stay conservative
    "p4": (65, 65, 4, 1, False, 0, (torch.arange(65) % 3).int(), None),
    # 5 q rows whose id no key has; kv rows 128..191 whose id no query has
    "p5": (64, 192, 4, 2, False, 0, _p5_q(), _docs(128, 64, first=0) * 5),
    # 4 docs of 64: every off-diagonal tile skipped
    "p6": (256, 256, 4, 2, True, 0, _docs(64, 64, 64, 64), None),
}
PARAMS = [(n, d) for n in CASES for d in (64, 128)]


def _seg(name):
    """(q_seg [B, Sq], kv_seg [B, Sk]) on the GPU, int32."""
    Sq, Sk, _, _, _, _, qi, ki = CASES[name]
    ki = qi if ki is None else ki
    assert qi.shape == (Sq,) and ki.shape == (Sk,)
    return (qi.cuda().expand(B, Sq).contiguous(), ki.cuda().expand(B, Sk).contiguous())


def _arena_inputs(shapes, seed):
    """Tensors of `shapes` as contiguous slices of one all-NaN bf16 arena,
    each with >= PAD_ROWS rows of NaN on both sides; plus the arena and its
    outside-the-slices mask."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    D = shapes[0][-1]
    pad = PAD_ROWS * D
    total = pad + sum(math.prod(s) + pad for s in shapes)
    arena = torch.full((total,), float("nan"), device="cuda", dtype=torch.bfloat16)
    outside = torch.ones(total, dtype=torch.bool, device="cuda")
    views, off = [], pad
    for s in shapes:
        n = math.prod(s)
        arena[off:off + n] = torch.randn(n, device="cuda", generator=g).bfloat16()
        outside[off:off + n] = False
        views.append(arena[off:off + n].view(s))
        off += n + pad
    return views, arena, outside, g


def _fwd_bwd(fn, q, k, v, dout, dlse):
    """(o, lse, dq, dk, dv) of fn under grads (dout, dlse) for (o, lse).
    The leaves share q/k/v's storage (detach, no clone), so the kernels get
    the arena slices themselves."""
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    o, lse = fn(q, k, v)
    dq, dk, dv = torch.autograd.grad([o, lse], [q, k, v], [dout.to(o.dtype), dlse])
    return tuple(t.detach() for t in (o, lse, dq, dk, dv))


def _flash(causal, shift, q_seg=None, kv_seg=None):
    from vescale_amd.ops import flash_attention

    return lambda a, b, c: flash_attention(
        a, b, c, is_causal=causal, causal_shift=shift, return_lse=True,
        q_segment_ids=q_seg, kv_segment_ids=kv_seg)


def _refs(q, k, v, dout, dlse, causal, shift, q_seg, kv_seg):
    """The reference in fp32 and with matmuls and softmax in bf16."""
    from vescale_amd.ops.functional import _attention_ref

    sc = 1.0 / math.sqrt(q.shape[-1])
    x32 = _fwd_bwd(lambda a, b, c: _attention_ref(
        a, b, c, causal, shift, sc, q_seg=q_seg, kv_seg=kv_seg),
        q.float(), k.float(), v.float(), dout.float(), dlse)
    x16 = _fwd_bwd(lambda a, b, c: _attention_ref(
        a, b, c, causal, shift, sc, dtype=torch.bfloat16, q_seg=q_seg, kv_seg=kv_seg),
        q, k, v, dout, dlse)
    return x32, x16


@functools.lru_cache(maxsize=None)
def _results(name, D):
    Sq, Sk, Hq, Hkv, causal, shift, _, _ = CASES[name]
    (q, k, v, dout), arena, outside, g = _arena_inputs(
        [(B, Hq, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D), (B, Hq, Sq, D)],
        2000 * sorted(CASES).index(name) + D)
    dlse = torch.randn(B, Hq, Sq, device="cuda", generator=g)
    q_seg, kv_seg = _seg(name)
    lo = arena.data_ptr()
    hi = lo + arena.numel() * arena.element_size()
    for t in (q, k, v, dout):
        # contiguous, so flash_attention's .contiguous() hands the kernel
        # this very pointer, NaN rows on both sides
        assert t.is_contiguous()
        pad_bytes = PAD_ROWS * D * t.element_size()
        assert lo + pad_bytes <= t.data_ptr()
        assert t.data_ptr() + t.numel() * t.element_size() + pad_bytes <= hi
    x = _fwd_bwd(_flash(causal, shift, q_seg, kv_seg), q, k, v, dout, dlse)
    torch.cuda.synchronize()
    arena_ok = bool((arena.view(torch.int16)[outside] == NAN_BITS).all())
    x32, x16 = _refs(q, k, v, dout, dlse, causal, shift, q_seg, kv_seg)
    return dict(x=x, x32=x32, x16=x16, arena_ok=arena_ok,
                inputs=(q, k, v, dout, dlse), seg=(q_seg, kv_seg))


def _check_bound(x, x32, x16, what):
    for i, nm in ((0, "o"), (2, "dq"), (3, "dk"), (4, "dv")):
        err = (x[i].float() - x32[i]).abs().max().item()
        e16 = (x16[i].float() - x32[i]).abs().max().item()
        tol = 2 * e16 + 2.0 ** -8 * x32[i].abs().max().item()
        print(f"{what} {nm}: err {err:.3e} e16 {e16:.3e} tol {tol:.3e}")
        assert err <= tol, (what, nm, err, e16, tol)


def _check_lse(lse, lse32, what):
    live = lse32 > float("-inf")
    assert torch.equal(lse > float("-inf"), live)
    if live.any():
        d = (lse[live] - lse32[live]).abs().max().item()
        print(f"{what} lse: err {d:.3e}")
        assert d <= 1e-2, d


@pytest.mark.parametrize("name,D", PARAMS)
def test_accuracy(name, D):
    r = _results(name, D)
    x, x32, x16 = r["x"], r["x32"], r["x16"]
    assert x[0].dtype == torch.bfloat16 and x[1].dtype == torch.float32
    _check_bound(x, x32, x16, f"{name}/D{D}")
    _check_lse(x[1], x32[1], f"{name}/D{D}")


@pytest.mark.parametrize("D", (64, 128))
def test_dead_rows_exact(D):
    o, lse, dq, dk, dv = _results("p5", D)["x"]
    dead = torch.zeros(64, dtype=torch.bool, device="cuda")
    dead[20:25] = True
    assert (o[:, :, dead] == 0).all()
    assert (lse[:, :, dead] == float("-inf")).all()
    assert (dq[:, :, dead] == 0).all()
    assert torch.isfinite(lse[:, :, ~dead]).all()
    # keys no query sees
    assert (dk[:, :, 128:] == 0).all() and (dv[:, :, 128:] == 0).all()
    assert (dk[:, :, :128] != 0).any() and (dv[:, :, :128] != 0).any()


@pytest.mark.parametrize("name,D", PARAMS)
def test_tails_never_read_or_written(name, D):
    """A tail row (or a segment id past the end) read as data would turn the
    results NaN or wrong; a store past a tensor would break the arena's NaN
    pattern."""
    r = _results(name, D)
    o, lse, dq, dk, dv = r["x"]
    for t in (o, dq, dk, dv):
        assert torch.isfinite(t.float()).all()
    assert not torch.isnan(lse).any()
    assert r["arena_ok"]


@pytest.mark.parametrize("name,D", [(n, d) for n in ("p1", "p6") for d in (64, 128)])
def test_packed_equals_separate(name, D):
    """Each document's slice of the packed results against flash_attention on
    that document alone: both meet the bound with the packed reference's
    slice as x32 (and the packed bf16 reference's slice as x16)."""
    Sq, Sk, Hq, Hkv, causal, shift, ids, _ = CASES[name]
    r = _results(name, D)
    q, k, v, dout, dlse = r["inputs"]
    edges = [0] + (torch.nonzero(ids[1:] != ids[:-1]).flatten() + 1).tolist() + [Sq]
    assert len(edges) == 5
    for a, b in zip(edges[:-1], edges[1:]):
        cut = lambda t: t[:, :, a:b]
        sl = lambda xs: tuple(cut(t) for t in xs)
        alone = _fwd_bwd(_flash(causal, 0),
                         *(cut(t).contiguous() for t in (q, k, v, dout, dlse)))
        x32, x16 = sl(r["x32"]), sl(r["x16"])
        _check_bound(alone, x32, x16, f"{name}/D{D} doc [{a},{b}) alone")
        _check_bound(sl(r["x"]), x32, x16, f"{name}/D{D} doc [{a},{b}) packed")
        _check_lse(alone[1], x32[1], f"{name}/D{D} doc [{a},{b}) alone")


@pytest.mark.parametrize("causal", (True, False))
@pytest.mark.parametrize("D", (64, 128))
def test_neutral_segments_bitwise(D, causal):
    """All ids equal: the SEG kernels give, bit for bit, what the kernels
    without a segment mask give."""
    q, k, v, dout, dlse = _results("p1", D)["inputs"]
    zero = torch.zeros(B, 130, dtype=torch.int32, device="cuda")
    plain = _fwd_bwd(_flash(causal, 0), q, k, v, dout, dlse)
    seg = _fwd_bwd(_flash(causal, 0, zero, zero), q, k, v, dout, dlse)
    for nm, a, b in zip(("o", "lse", "dq", "dk", "dv"), plain, seg):
        assert torch.equal(a, b), nm


def test_repeatable():
    for D in (64, 128):
        r = _results("p1", D)
        q, k, v, dout, dlse = r["inputs"]
        fn = _flash(True, 0, *r["seg"])
        r1 = _fwd_bwd(fn, q, k, v, dout, dlse)
        r2 = _fwd_bwd(fn, q, k, v, dout, dlse)
        for a, b in zip(r1, r2):
            assert torch.equal(a, b)
        for a, b in zip(r1, r["x"]):
            assert torch.equal(a, b)


def test_dispatch_segments_take_the_general_kernels():
    """At a shape the tuned D=128 kernels accept, a call with segment ids
    does not take them (it would lose the mask); without ids it still does."""
    from vescale_amd.ops import flash_attention, flash_attention_causal

    S, D = 512, 128
    g = torch.Generator(device="cuda").manual_seed(5)
    q = torch.randn(B, 4, S, D, device="cuda", generator=g).bfloat16()
    k = torch.randn(B, 2, S, D, device="cuda", generator=g).bfloat16()
    v = torch.randn(B, 2, S, D, device="cuda", generator=g).bfloat16()
    dout = torch.randn(B, 4, S, D, device="cuda", generator=g).bfloat16()
    seg = _docs(200, 312).cuda().expand(B, S).contiguous()
    tuned = flash_attention_causal(q, k, v)
    assert torch.equal(flash_attention(q, k, v, is_causal=True), tuned)
    assert not torch.equal(flash_attention(q, k, v, is_causal=True, q_segment_ids=seg), tuned)
    zero = torch.zeros(B, 4, S, device="cuda")
    x = _fwd_bwd(_flash(True, 0, seg), q, k, v, dout, zero)
    x32, x16 = _refs(q, k, v, dout, zero, True, 0, seg, seg)
    _check_bound(x, x32, x16, "dispatch")
    _check_lse(x[1], x32[1], "dispatch")
