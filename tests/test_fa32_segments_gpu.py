"""Packed-document mask of the tuned 32x32 flash kernels (SEG instantiations of
attention_fwd.hip / attention_bwd2.hip) through the public
flash_attention(..., contiguous_segments=True), by the method and the bound of
test_flash_attention_segments_gpu.py, for every tensor x of o, dq, dk, dv:

    max|x - x32| <= 2 * max|x16 - x32| + 2^-8 * max|x32|

with x32 / x16 the torch reference in fp32 / bf16 given the canonical run ids.
The two batch rows carry different layouts (the second row's documents in
reverse order), so a wrong batch stride in the bounds shows.
"""
import functools
import math

import pytest
import torch


def gpu(f):
    """The GPU tests' marks; the CPU tests at the end of the file carry none."""
    return pytest.mark.gpu(
        pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")(f))


@pytest.fixture(autouse=True)
def _no_intra_op_pool():
    """As in test_flash_attention_general.py: the in-process math of the CPU
    tests must not start the intra-op thread pool, later files fork this process."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


B, HQ, HKV, D = 2, 4, 2, 128
SCALE = 1.0 / math.sqrt(D)


def _ids(lengths, names=None):
    names = range(len(lengths)) if names is None else names
    return torch.cat([torch.full((n,), d, dtype=torch.int32) for d, n in zip(names, lengths)])


# name: (S, document lengths of row 0, their ids or None = 0, 1, 2, ...)
CASES = {
    "off_edges": (512, (200, 312), None),
    "on_edges": (512, (64, 64, 128, 256), None),
    "in_one_wave": (512, (1, 30, 33, 64, 2, 126, 256), None),
    "spans_blocks": (1024, (300, 724), None),
    "reappearing": (512, (100, 156, 256), (0, 1, 0)),
}


def _run_ids(ids):
    """Canonical run ids with plain torch: the first position of each run."""
    edge = torch.ones_like(ids, dtype=torch.bool)
    edge[:, 1:] = ids[:, 1:] != ids[:, :-1]
    pos = torch.arange(ids.shape[1], device=ids.device).expand_as(ids)
    return torch.cummax(torch.where(edge, pos, 0), 1).values.int()


def _fwd_bwd(fn, q, k, v, dout):
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    o = fn(q, k, v)
    return (o.detach(), *(g.detach() for g in torch.autograd.grad(o, [q, k, v], dout.to(o.dtype))))


def _packed(ids, **kw):
    from vescale_amd.ops import flash_attention
    return lambda a, b, c: flash_attention(a, b, c, is_causal=True, q_segment_ids=ids, **kw)


@functools.lru_cache(maxsize=None)
def _results(name):
    from vescale_amd.ops.functional import _attention_ref
    S, lengths, names = CASES[name]
    ids = torch.stack([_ids(lengths, names), _ids(lengths[::-1], names)]).cuda()
    assert ids.shape == (B, S)
    g = torch.Generator(device="cuda").manual_seed(sorted(CASES).index(name))
    q, dout = (torch.randn(B, HQ, S, D, device="cuda", generator=g).bfloat16() for _ in range(2))
    k, v = (torch.randn(B, HKV, S, D, device="cuda", generator=g).bfloat16() for _ in range(2))
    run = _run_ids(ids)
    ref = lambda dt: lambda a, b, c: _attention_ref(a, b, c, True, 0, SCALE, dtype=dt,
                                                    q_seg=run, kv_seg=run)[0]
    return dict(ids=ids, inputs=(q, k, v, dout),
                x=_fwd_bwd(_packed(ids, contiguous_segments=True), q, k, v, dout),
                x32=_fwd_bwd(ref(None), q.float(), k.float(), v.float(), dout.float()),
                x16=_fwd_bwd(ref(torch.bfloat16), q, k, v, dout))


def _check_bound(x, x32, x16, what):
    for nm, a, a32, a16 in zip(("o", "dq", "dk", "dv"), x, x32, x16):
        assert not torch.isnan(a).any(), (what, nm)
        err = (a.float() - a32).abs().max().item()
        e16 = (a16.float() - a32).abs().max().item()
        tol = 2 * e16 + 2.0 ** -8 * a32.abs().max().item()
        print(f"{what} {nm}: err {err:.3e} e16 {e16:.3e} tol {tol:.3e}")
        assert err <= tol, (what, nm, err, e16, tol)


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_accuracy(name):
    r = _results(name)
    _check_bound(r["x"], r["x32"], r["x16"], name)
    if name == "reappearing":  # a reappearing id is a new document, not the old one
        eq = _fwd_bwd(_packed(r["ids"]), *r["inputs"])
        assert not torch.equal(eq[0], r["x"][0])


@gpu
def test_one_document_bitwise():
    """All ids equal: nothing masked beyond causal, nothing skipped."""
    from vescale_amd.ops import flash_attention_causal
    q, k, v, dout = _results("off_edges")["inputs"]
    seg = _fwd_bwd(_packed(torch.full((B, 512), 3, device="cuda"), contiguous_segments=True),
                   q, k, v, dout)
    for nm, a, b in zip(("o", "dq", "dk", "dv"), _fwd_bwd(flash_attention_causal, q, k, v, dout), seg):
        assert torch.equal(a, b), nm


@gpu
@pytest.mark.parametrize("name", ("off_edges", "on_edges"))
def test_packed_equals_separate(name):
    from vescale_amd.ops import flash_attention
    r = _results(name)
    for row in range(B):
        lengths = CASES[name][1][::-1] if row else CASES[name][1]
        edges = [0] + torch.tensor(lengths).cumsum(0).tolist()
        for a, b in zip(edges[:-1], edges[1:]):
            sl = lambda xs: tuple(t[row:row + 1, :, a:b] for t in xs)
            # return_lse keeps a 256-long document on the general kernels too
            alone = _fwd_bwd(lambda x, y, z: flash_attention(x, y, z, is_causal=True,
                                                             return_lse=True)[0],
                             *(t.contiguous() for t in sl(r["inputs"])))
            _check_bound(alone, sl(r["x32"]), sl(r["x16"]), f"{name} row {row} [{a},{b}) alone")
            _check_bound(sl(r["x"]), sl(r["x32"]), sl(r["x16"]), f"{name} row {row} [{a},{b}) packed")


@gpu
def test_repeatable():
    r = _results("in_one_wave")
    again = _fwd_bwd(_packed(r["ids"], contiguous_segments=True), *r["inputs"])
    for a, b in zip(r["x"], again):
        assert torch.equal(a, b)


@gpu
def test_binding_returns_run_bounds():
    """fa_fwd(.., segment_ids=) hands back the bounds only the tuned path makes."""
    import vescale_amd.ops as ops
    r = _results("in_one_wave")
    q, k, v, _ = r["inputs"]
    out, lse, bounds = ops._C.fa_fwd(q, k, v, SCALE, segment_ids=r["ids"])
    start = _run_ids(r["ids"])
    end = 512 - _run_ids(r["ids"].flip(1)).flip(1)
    assert torch.equal(bounds, torch.stack([start, end], 1))
    assert lse.isfinite().all()  # every row sees its own diagonal
    assert torch.equal(out, r["x"][0])


def _dense(q, k, v, ids):
    """Masked softmax with the run mask written out, fp32."""
    S = q.shape[2]
    run = _run_ids(ids)
    vis = (run[:, :, None] == run[:, None, :]) & torch.ones(S, S, dtype=torch.bool).tril()
    s = (q @ k.transpose(-1, -2)) * (q.shape[-1] ** -0.5)
    return torch.softmax(s.masked_fill(~vis[:, None], float("-inf")), -1) @ v


@pytest.mark.parametrize("ids", ([0] * 5 + [1] * 11, [4] * 3 + [9] * 6 + [4] * 7))
def test_cpu_run_semantics(ids):
    from vescale_amd.ops import flash_attention
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(2, 2, 16, 8, generator=g) for _ in range(3))
    ids = torch.tensor([ids, ids[::-1]])
    o = flash_attention(q, k, v, is_causal=True, q_segment_ids=ids, contiguous_segments=True)
    assert torch.allclose(o, _dense(q, k, v, ids), atol=1e-5)


@pytest.mark.parametrize("kw", (dict(is_causal=False), dict(causal_shift=1), dict(kv=True),
                                dict(sk=8), dict(no_ids=True)))
def test_contiguous_segments_rules(kw):
    from vescale_amd.ops import flash_attention
    q = torch.zeros(1, 1, 16, 8)
    kv = torch.zeros(1, 1, kw.get("sk", 16), 8)
    ids = torch.zeros(1, 16, dtype=torch.int32)
    with pytest.raises(ValueError):
        flash_attention(q, kv, kv, is_causal=kw.get("is_causal", True),
                        causal_shift=kw.get("causal_shift", 0), contiguous_segments=True,
                        q_segment_ids=None if kw.get("no_ids") else ids,
                        kv_segment_ids=torch.zeros(1, kv.shape[2], dtype=torch.int32)
                        if kw.get("kv") or kw.get("sk") else None)
