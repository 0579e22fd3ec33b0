"""General-shape flash attention kernel (ops/csrc/attention_gen.hip) on the
GPU: accuracy against the fp32 torch reference with the same-precision eager
computation as the yardstick, dead rows, tails (NaN arena), repeatability,
blockwise (ring-style) composition and dispatch.

Accuracy bound, every tensor x of o, dq, dk, dv:

    max|x - x32| <= 2 * max|x16 - x32| + 2^-8 * max|x32|

x32 is the torch reference in fp32, x16 the same reference with matmuls and
softmax in bf16.  The factor 2 is the customary margin of a flash kernel
over the same-precision eager computation (its summation order differs, its
precision does not); the second term is one bf16 ulp at the largest output,
so exact cases (Sq = Sk = 1) do not demand zero error.
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

# name: (Sq, Sk, Hq, Hkv, causal, shift)
CASES = {
    "a_nc": (1, 1, 2, 2, False, 0),
    "a_c": (1, 1, 2, 2, True, 0),
    "b": (63, 63, 4, 2, False, 0),
    "c": (65, 65, 4, 2, True, 0),
    "d": (130, 130, 4, 1, True, 0),
    "e_nc": (70, 200, 4, 2, False, 0),
    "e_br": (70, 200, 4, 2, True, 130),
    "e_tl": (70, 200, 4, 2, True, 0),
    "f_m5": (64, 192, 4, 2, True, -5),
    "f_m64": (64, 192, 4, 2, True, -64),
    "g": (256, 256, 4, 2, True, 0),
}
PARAMS = [(n, d) for n in CASES for d in (64, 128) if not (n == "g" and d == 64)]
NAN_BITS = torch.tensor(float("nan"), dtype=torch.bfloat16).view(torch.int16).item()


def _arena_inputs(name, D):
    """q, k, v, dout as contiguous slices of one all-NaN bf16 arena, each
    with >= PAD_ROWS rows of NaN on both sides; plus dlse and the arena's
    outside-the-slices mask."""
    Sq, Sk, Hq, Hkv, _, _ = CASES[name]
    g = torch.Generator(device="cuda").manual_seed(
        1000 * sorted(CASES).index(name) + D)
    shapes = [(B, Hq, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D), (B, Hq, Sq, D)]
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
    dlse = torch.randn(B, Hq, Sq, device="cuda", generator=g)
    return views, dlse, arena, outside


def _fwd_bwd(fn, q, k, v, dout, dlse):
    """(o, lse, dq, dk, dv) of fn under grads (dout, dlse) for (o, lse).
    The leaves share q/k/v's storage (detach, no clone), so the kernels get
    the arena slices themselves."""
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    o, lse = fn(q, k, v)
    dq, dk, dv = torch.autograd.grad([o, lse], [q, k, v], [dout.to(o.dtype), dlse])
    return tuple(t.detach() for t in (o, lse, dq, dk, dv))


@functools.lru_cache(maxsize=None)
def _results(name, D):
    from vescale_amd.ops import flash_attention
    from vescale_amd.ops.functional import _attention_ref

    Sq, Sk, Hq, Hkv, causal, shift = CASES[name]
    sc = 1.0 / math.sqrt(D)
    (q, k, v, dout), dlse, arena, outside = _arena_inputs(name, D)
    lo = arena.data_ptr()
    hi = lo + arena.numel() * arena.element_size()
    for t in (q, k, v, dout):
        # contiguous, so flash_attention's .contiguous() hands the kernel
        # this very pointer, NaN rows on both sides
        assert t.is_contiguous()
        assert t.detach().data_ptr() == t.data_ptr()
        pad_bytes = PAD_ROWS * D * t.element_size()
        assert lo + pad_bytes <= t.data_ptr()
        assert t.data_ptr() + t.numel() * t.element_size() + pad_bytes <= hi
    x = _fwd_bwd(lambda a, b, c: flash_attention(
        a, b, c, is_causal=causal, causal_shift=shift, return_lse=True),
        q, k, v, dout, dlse)
    torch.cuda.synchronize()
    arena_ok = bool((arena.view(torch.int16)[outside] == NAN_BITS).all())
    x32 = _fwd_bwd(lambda a, b, c: _attention_ref(a, b, c, causal, shift, sc),
                   q.float(), k.float(), v.float(), dout.float(), dlse)
    x16 = _fwd_bwd(lambda a, b, c: _attention_ref(
        a, b, c, causal, shift, sc, dtype=torch.bfloat16), q, k, v, dout, dlse)
    return dict(x=x, x32=x32, x16=x16, arena_ok=arena_ok,
                inputs=(q, k, v, dout, dlse))


def _check_bound(x, x32, x16, what):
    for i, nm in ((0, "o"), (2, "dq"), (3, "dk"), (4, "dv")):
        err = (x[i].float() - x32[i]).abs().max().item()
        e16 = (x16[i].float() - x32[i]).abs().max().item()
        tol = 2 * e16 + 2.0 ** -8 * x32[i].abs().max().item()
        print(f"{what} {nm}: err {err:.3e} e16 {e16:.3e} tol {tol:.3e}")
        assert err <= tol, (what, nm, err, e16, tol)


@pytest.mark.parametrize("name,D", PARAMS)
def test_accuracy(name, D):
    r = _results(name, D)
    x, x32, x16 = r["x"], r["x32"], r["x16"]
    assert x[0].dtype == torch.bfloat16 and x[1].dtype == torch.float32
    _check_bound(x, x32, x16, f"{name}/D{D}")
    live = x32[1] > float("-inf")
    assert torch.equal(x[1] > float("-inf"), live)
    if live.any():
        d = (x[1][live] - x32[1][live]).abs().max().item()
        print(f"{name}/D{D} lse: err {d:.3e}")
        assert d <= 1e-2, d


@pytest.mark.parametrize("name,D", PARAMS)
def test_dead_rows_exact(name, D):
    Sq, Sk, Hq, Hkv, causal, shift = CASES[name]
    o, lse, dq, dk, dv = _results(name, D)["x"]
    dead = torch.arange(Sq, device="cuda") + shift < 0 if causal else \
        torch.zeros(Sq, dtype=torch.bool, device="cuda")
    if name == "f_m5":
        assert int(dead.sum()) == 5
    if name == "f_m64":
        assert bool(dead.all())
    assert (o[:, :, dead] == 0).all()
    assert (lse[:, :, dead] == float("-inf")).all()
    assert (dq[:, :, dead] == 0).all()
    assert torch.isfinite(lse[:, :, ~dead]).all()
    # dk/dv can be checked for exact zeros only where every row is dead
    # (f_m64).  With some rows dead (f_m5) their contribution to dk/dv is
    # covered by test_accuracy: dout and dlse are random on the dead rows
    # too, so a leak of either into dk/dv breaks the bound there.
    if bool(dead.all()):
        assert (dk == 0).all() and (dv == 0).all()


@pytest.mark.parametrize("name,D", PARAMS)
def test_tails_never_read_or_written(name, D):
    """A tail row read as data would turn the results NaN; a store past a
    tensor would break the arena's NaN pattern."""
    r = _results(name, D)
    o, lse, dq, dk, dv = r["x"]
    for t in (o, dq, dk, dv):
        assert torch.isfinite(t.float()).all()
    assert not torch.isnan(lse).any()
    assert r["arena_ok"]


def test_matches_tuned_kernels():
    """Case g: the general and the tuned D=128 kernels both meet the bound
    against the fp32 reference on a shape both accept."""
    import vescale_amd.ops as ops

    C = ops.require_ext()
    r = _results("g", 128)
    q, k, v, dout, _ = r["inputs"]
    q, k, v, dout = (t.contiguous() for t in (q, k, v, dout))
    sc = 1.0 / math.sqrt(128)
    from vescale_amd.ops.functional import _attention_ref

    def ref(dtype):
        def fn(a, b, c):
            o, lse = _attention_ref(a, b, c, True, 0, sc, dtype=dtype)
            return o, lse
        return fn

    zero = torch.zeros_like(r["x"][1])
    x32 = _fwd_bwd(ref(None), q.float(), k.float(), v.float(), dout.float(), zero)
    x16 = _fwd_bwd(ref(torch.bfloat16), q, k, v, dout, zero)
    o_g, lse_g = C.fa_gen_fwd(q, k, v, sc, True, 0)
    gen = (o_g, lse_g) + tuple(C.fa_gen_bwd(q, k, v, o_g, dout, lse_g, None, sc, True, 0))
    o_t, lse_t = C.fa_fwd(q, k, v, sc)
    tuned = (o_t, lse_t) + tuple(C.fa_bwd2(q, k, v, o_t, dout, lse_t, sc, False))
    _check_bound(gen, x32, x16, "g general")
    _check_bound(tuned, x32, x16, "g tuned")
    assert (lse_g - x32[1]).abs().max().item() <= 1e-2
    assert (lse_t - x32[1]).abs().max().item() <= 1e-2


def test_repeatable():
    from vescale_amd.ops import flash_attention

    for D in (64, 128):
        q, k, v, dout, dlse = _results("d", D)["inputs"]
        fn = lambda a, b, c: flash_attention(a, b, c, is_causal=True, return_lse=True)
        r1 = _fwd_bwd(fn, q, k, v, dout, dlse)
        r2 = _fwd_bwd(fn, q, k, v, dout, dlse)
        for a, b in zip(r1, r2):
            assert torch.equal(a, b)


@pytest.mark.parametrize("D", (64, 128))
def test_blockwise_composition(D):
    """The ring's math on one GPU: case d's K/V in chunks of 64, 64 and 2
    rows, each a flash_attention call with causal_shift = -chunk_start,
    merged as ring_sdpa merges; exercises dlse and dead rows under real
    merging."""
    from vescale_amd.dmodule.ring_attention import _merge
    from vescale_amd.ops import flash_attention

    r = _results("d", D)
    q, k, v, dout, _ = r["inputs"]
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    acc = lse = None
    for start, end in ((0, 64), (64, 128), (128, 130)):
        o_b, l_b = flash_attention(q, k[:, :, start:end], v[:, :, start:end],
                                   is_causal=True, causal_shift=-start,
                                   return_lse=True)
        o_b, l_b = o_b.float(), l_b.unsqueeze(-1)
        if acc is None:
            acc, lse = o_b, l_b
        else:
            acc, lse = _merge(acc, lse, o_b, l_b)
    out = acc.to(torch.bfloat16)
    dq, dk, dv = torch.autograd.grad(out, [q, k, v], dout)
    got = (out.detach(), lse.squeeze(-1).detach(), dq, dk, dv)
    for t in got:
        assert torch.isfinite(t.float()).all()
    # references with the out-only loss (no dlse)
    from vescale_amd.ops.functional import _attention_ref

    sc = 1.0 / math.sqrt(D)
    zero = torch.zeros_like(r["x"][1])
    qi, ki, vi = r["inputs"][:3]
    x32 = _fwd_bwd(lambda a, b, c: _attention_ref(a, b, c, True, 0, sc),
                   qi.float(), ki.float(), vi.float(), dout.float(), zero)
    x16 = _fwd_bwd(lambda a, b, c: _attention_ref(
        a, b, c, True, 0, sc, dtype=torch.bfloat16), qi, ki, vi, dout, zero)
    _check_bound(got, x32, x16, f"blockwise/D{D}")
    assert (got[1] - x32[1]).abs().max().item() <= 1e-2


def test_dispatch_tuned_path_kept():
    from vescale_amd.ops import flash_attention, flash_attention_causal

    g = torch.Generator(device="cuda").manual_seed(5)
    q = torch.randn(2, 4, 512, 128, device="cuda", generator=g).bfloat16()
    k = torch.randn(2, 2, 512, 128, device="cuda", generator=g).bfloat16()
    v = torch.randn(2, 2, 512, 128, device="cuda", generator=g).bfloat16()
    a = flash_attention(q, k, v, is_causal=True)
    b = flash_attention_causal(q, k, v)
    assert torch.equal(a, b)


def test_dispatch_aten_escape_hatch(monkeypatch):
    from vescale_amd.ops import flash_attention

    name, D = "c", 64
    Sq, Sk, Hq, Hkv, causal, shift = CASES[name]
    r = _results(name, D)
    q, k, v, dout, dlse = r["inputs"]
    monkeypatch.setenv("VESCALE_FA", "aten")
    xa = _fwd_bwd(lambda a, b, c: flash_attention(
        a, b, c, is_causal=causal, causal_shift=shift, return_lse=True),
        q, k, v, dout, dlse)
    x, x32, x16 = r["x"], r["x32"], r["x16"]
    for i, nm in ((0, "o"), (2, "dq"), (3, "dk"), (4, "dv")):
        err = (x[i].float() - xa[i].float()).abs().max().item()
        e16 = (x16[i].float() - x32[i]).abs().max().item()
        tol = 2 * e16 + 2.0 ** -8 * x32[i].abs().max().item()
        assert err <= tol, (nm, err, tol)
