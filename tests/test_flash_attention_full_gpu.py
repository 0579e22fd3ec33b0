"""The tuned 32x32 flash kernels' FULL (no mask, Sq != Sk) instantiations and
differentiable lse on the GPU, through flash_attention; method, helpers and
bounds of test_flash_attention_segments_gpu.py (x32 / x16: _attention_ref)."""
import functools

import pytest
import torch

import vescale_amd.ops as ops
from tests.test_flash_attention_segments_gpu import (
    B, NAN_BITS, _arena_inputs, _check_bound, _check_lse, _fwd_bwd)
from vescale_amd.dmodule.ring_attention import _merge
from vescale_amd.ops.functional import _attention_ref

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")]

D, SC = 128, 128 ** -0.5
# name: (Sq, Sk, Hq, Hkv, is_causal, return_lse)
CASES = {
    "square": (256, 256, 4, 2, False, True),
    "wide": (256, 512, 4, 2, False, True),     # kbase by Sk; batch stride (B = 2)
    "tall": (512, 256, 4, 1, False, True),     # MQA; dq grid > dv/dk grid; reduce over Sk
    "outonly": (512, 512, 4, 4, False, False),  # no lse; Hkv == Hq: no reduce
    "causal": (512, 512, 4, 2, True, True),    # the causal kernels, lse and dlse
}


def _flash(causal, want_lse, q, k, v):
    # without return_lse: a zero lse that hangs on o, so one _fwd_bwd serves both
    r = ops.flash_attention(q, k, v, is_causal=causal, return_lse=want_lse)
    return r if want_lse else (r, r.float().sum(-1) * 0)


def _refs(q, k, v, dout, dlse, causal, want_lse):
    def ref(a, b, c, dt=None):
        o, lse = _attention_ref(a, b, c, causal, 0, SC, dtype=dt)
        return o, lse if want_lse else lse * 0
    return (_fwd_bwd(ref, q.float(), k.float(), v.float(), dout.float(), dlse),
            _fwd_bwd(functools.partial(ref, dt=torch.bfloat16), q, k, v, dout, dlse))


@functools.lru_cache(maxsize=None)
def _results(name):
    Sq, Sk, Hq, Hkv, causal, want_lse = CASES[name]
    (q, k, v, dout), arena, outside, g = _arena_inputs(
        [(B, Hq, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D), (B, Hq, Sq, D)],
        4000 * sorted(CASES).index(name) + D)
    dlse = torch.randn(B, Hq, Sq, device="cuda", generator=g)
    x = _fwd_bwd(functools.partial(_flash, causal, want_lse), q, k, v, dout, dlse)
    torch.cuda.synchronize()
    arena_ok = bool((arena.view(torch.int16)[outside] == NAN_BITS).all())
    x32, x16 = _refs(q, k, v, dout, dlse, causal, want_lse)
    return dict(x=x, x32=x32, x16=x16, arena_ok=arena_ok, inputs=(q, k, v, dout, dlse))


@pytest.mark.parametrize("name", CASES)
def test_accuracy_and_arena(name):
    r = _results(name)
    _check_bound(r["x"], r["x32"], r["x16"], name)
    _check_lse(r["x"][1], r["x32"][1], name)
    assert all(torch.isfinite(t.float()).all() for t in r["x"]) and r["arena_ok"]


@pytest.mark.parametrize("name", CASES)
def test_dispatch_and_bitwise(name, monkeypatch):
    """bitwise the tuned bindings (both layouts of o / dout), not the general
    kernels; repeatable"""
    causal, want_lse = CASES[name][4:]
    r = _results(name)
    q, k, v, dout, dlse = r["inputs"]
    o, lse, dq, dk, dv = r["x"]
    same = lambda xs, ys: all(torch.equal(a, b) for a, b in zip(xs, ys))
    C, kw = ops.require_ext(), dict(causal=causal, dlse=dlse if want_lse else None)
    o_c, lse_c = C.fa_fwd(q, k, v, SC, causal=causal)
    assert torch.equal(o, o_c) and (not want_lse or torch.equal(lse, lse_c))
    g = C.fa_bwd2(q, k, v, o_c, dout, lse_c, SC, False, **kw)
    assert same(g, (dq, dk, dv))
    o_b = C.fa_fwd(q, k, v, SC, out_bshd=True, causal=causal)[0]
    assert torch.equal(o_b.transpose(1, 2), o_c)
    assert same(g, C.fa_bwd2(q, k, v, o_b, dout.transpose(1, 2).contiguous(), lse_c, SC,
                             False, bshd=True, **kw))
    if causal:  # dlse = 0 is no dlse
        assert same(C.fa_bwd2(q, k, v, o_c, dout, lse_c, SC, False, dlse=torch.zeros_like(dlse)),
                    C.fa_bwd2(q, k, v, o_c, dout, lse_c, SC, False))
    again = lambda: _fwd_bwd(functools.partial(_flash, causal, want_lse), q, k, v, dout, dlse)
    assert same(again(), r["x"])
    monkeypatch.setenv("VESCALE_FA_FULL", "gen")
    gen = again()
    assert not torch.equal(gen[0], o) and not torch.equal(gen[2], dq)


def test_blockwise_composition():
    """The ring's math on one GPU, S = 512 causal as two blocks of 256: real
    dlse through the FULL and the causal path, merged as ring_sdpa merges."""
    q, k, v, dout, dlse = _results("causal")["inputs"]
    ql, kl, vl = (t.detach().requires_grad_(True) for t in (q, k, v))
    fl = lambda a, b, c, causal: ops.flash_attention(a, b, c, is_causal=causal, return_lse=True)
    lo, hi = slice(0, 256), slice(256, 512)
    o0, _ = fl(ql[:, :, lo], kl[:, :, lo], vl[:, :, lo], True)
    oa, la = fl(ql[:, :, hi], kl[:, :, lo], vl[:, :, lo], False)
    ob, lb = fl(ql[:, :, hi], kl[:, :, hi], vl[:, :, hi], True)
    o1, _ = _merge(oa.float(), la.unsqueeze(-1), ob.float(), lb.unsqueeze(-1))
    out = torch.cat([o0, o1.to(torch.bfloat16)], dim=2)
    dq, dk, dv = torch.autograd.grad(out, [ql, kl, vl], dout)
    x32, x16 = _refs(q, k, v, dout, torch.zeros_like(dlse), True, True)
    _check_bound((out.detach(), None, dq, dk, dv), x32, x16, "ring")
