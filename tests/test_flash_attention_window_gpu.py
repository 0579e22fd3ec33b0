"""The WIN (band-masked) instantiations of attention_gen.hip on the GPU, by
the method, helpers and bounds of test_flash_attention_segments_gpu.py, with
_attention_ref(lower=) in fp32 / bf16 as x32 / x16; the window reaches it by the
mapping that test_flash_attention_window.py holds to the dense definition."""
import functools

import pytest
import torch

from tests.test_flash_attention_segments_gpu import (
    B, NAN_BITS, _arena_inputs, _check_bound, _check_lse, _docs, _fwd_bwd)
from vescale_amd.ops import flash_attention, flash_attention_causal
from vescale_amd.ops.functional import _attention_ref, _window_args

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")]

# name: (Sq, Sk, Hq, Hkv, causal, shift, window, segment ids [S] or None)
CASES = {
    # band edge on / before / past a tile boundary: both tile bounds move by one.  e65 is MQA
    "e63": (260, 260, 4, 2, True, 0, (63, 0), None),
    "e64": (260, 260, 4, 2, True, 0, (64, 0), None),
    "e65": (260, 260, 4, 1, True, 0, (65, 0), None),
    "diag": (130, 130, 4, 2, True, 0, (0, 0), None),
    "band": (200, 200, 4, 2, False, 0, (70, 10), None),    # right folded into the shift
    "cross": (70, 200, 4, 2, True, 130, (40, 0), None),
    "dead": (200, 70, 4, 2, False, 0, (20, None), None),   # rows > 89 dead
    "seg4": (256, 256, 4, 2, True, 0, (100, 0), _docs(64, 64, 64, 64)),
    "segx": (256, 256, 4, 2, True, 0, (100, 0), _docs(1, 63, 2, 190)),
    "tuned": (512, 512, 4, 2, True, 0, (100, 0), None),    # the tuned kernels' gate
}


def _flash(causal, shift, window, seg=None, lse=True):
    return functools.partial(flash_attention, is_causal=causal, causal_shift=shift,
                             return_lse=lse, window=window, q_segment_ids=seg)


@functools.lru_cache(maxsize=None)
def _results(name, D):
    Sq, Sk, Hq, Hkv, causal, shift, window, ids = CASES[name]
    (q, k, v, dout), arena, outside, g = _arena_inputs(
        [(B, Hq, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D), (B, Hq, Sq, D)],
        3000 * sorted(CASES).index(name) + D)
    dlse = torch.randn(B, Hq, Sq, device="cuda", generator=g)
    seg = None if ids is None else ids.cuda().expand(B, Sq).contiguous()
    x = _fwd_bwd(_flash(causal, shift, window, seg), q, k, v, dout, dlse)
    torch.cuda.synchronize()
    arena_ok = bool((arena.view(torch.int16)[outside] == NAN_BITS).all())
    rc, rs, lower = _window_args(window, causal, shift)
    ref = lambda dt: lambda a, b, c: _attention_ref(
        a, b, c, rc, rs, D ** -0.5, dtype=dt, q_seg=seg, kv_seg=seg, lower=lower)
    x32 = _fwd_bwd(ref(None), q.float(), k.float(), v.float(), dout.float(), dlse)
    x16 = _fwd_bwd(ref(torch.bfloat16), q, k, v, dout, dlse)
    return dict(x=x, x32=x32, x16=x16, arena_ok=arena_ok, seg=seg,
                inputs=(q, k, v, dout, dlse))


@pytest.mark.parametrize("name,D", [(n, d) for n in CASES for d in (64, 128)])
def test_accuracy_and_tails(name, D):
    """The bound; tails never read (finite) or written (arena); dead rows;
    inside the tuned kernels' gate: no window, tuned; window, general"""
    r = _results(name, D)
    _check_bound(r["x"], r["x32"], r["x16"], f"{name}/D{D}")
    _check_lse(r["x"][1], r["x32"][1], f"{name}/D{D}")
    o, lse, dq, dk, dv = r["x"]
    assert all(torch.isfinite(t.float()).all() for t in (o, dq, dk, dv))
    assert not lse.isnan().any() and r["arena_ok"]
    if name == "dead":
        assert (o[:, :, 90:] == 0).all() and (dq[:, :, 90:] == 0).all()
        assert (lse[:, :, 90:] == float("-inf")).all() and lse[:, :, :90].isfinite().all()
    if (name, D) == ("tuned", 128):
        q, k, v = r["inputs"][:3]
        tuned = flash_attention_causal(q, k, v)
        assert torch.equal(_flash(True, 0, None, lse=False)(q, k, v), tuned)
        windowed = _flash(True, 0, (100, 0), lse=False)(q, k, v)
        assert not torch.equal(windowed, tuned) and torch.equal(windowed, o)


@pytest.mark.parametrize("with_ids", (False, True))
@pytest.mark.parametrize("D", (64, 128))
def test_neutral_window_bitwise_and_repeatable(D, with_ids):
    """left >= S: bitwise the call without a window; two runs: bitwise equal"""
    r = _results("segx", D)
    plain, wide = (_fwd_bwd(_flash(True, 0, w, r["seg"] if with_ids else None), *r["inputs"])
                   for w in (None, (256, 0)))
    again = _fwd_bwd(_flash(True, 0, (100, 0), r["seg"]), *r["inputs"])
    assert all(torch.equal(a, b) for a, b in zip(plain + again, wide + r["x"]))
