"""Binding contract of the layout keywords of the tuned flash attention
(fa_fwd out_bshd=, fa_bwd2 bshd=), exercised WITHOUT a device like
test_ext_contract.py: every call must end in a RuntimeError raised by host
validation, never in a HIP runtime error."""
import pytest
import torch

import vescale_amd.ops as ops

pytestmark = [
    pytest.mark.skipif(not ops.has_ext(), reason="needs the built extension"),
    pytest.mark.skipif(torch.cuda.is_available(),
                       reason="CPU-only: with a GPU a missed check reaches a kernel"),
]

BF, F32 = torch.bfloat16, torch.float32
B, HQ, HKV, S, D = 1, 2, 1, 256, 128  # Hq != S: the two layouts differ in shape


def T(*shape, dtype=BF):
    # uninitialised on purpose, see test_ext_contract.T
    return torch.empty(*shape, dtype=dtype)


def _qkv():
    return [T(B, HQ, S, D), T(B, HKV, S, D), T(B, HKV, S, D)]


def _bwd(o=(B, S, HQ, D), dout=(B, S, HQ, D), o_dtype=BF, dout_dtype=BF):
    return _qkv() + [T(*o, dtype=o_dtype), T(*dout, dtype=dout_dtype),
                     T(B, HQ, S, dtype=F32), 0.1, False]


def _rejected(name, args, **kw):
    with pytest.raises(RuntimeError) as ei:
        getattr(ops._C, name)(*args, **kw)
    msg = str(ei.value)
    assert "ROCm-capable" not in msg and "HIP error" not in msg, msg
    return msg


@pytest.mark.parametrize("flag", [False, True])
def test_keywords_are_accepted(flag):
    # well-formed CPU calls get past every argument check and stop at the launch
    msg = _rejected("fa_fwd", _qkv() + [0.1], out_bshd=flag)
    assert "fa_fwd: argument 'q' expected device=a GPU" in msg, msg
    shape = (B, S, HQ, D) if flag else (B, HQ, S, D)
    msg = _rejected("fa_bwd2", _bwd(o=shape, dout=shape), bshd=flag)
    assert "fa_bwd2: argument 'q' expected device=a GPU" in msg, msg


@pytest.mark.parametrize("arg", ["o", "dout"])
def test_bshd_rejects_the_bhsd_shape(arg):
    msg = _rejected("fa_bwd2", _bwd(**{arg: (B, HQ, S, D)}), bshd=True)
    assert f"fa_bwd2: argument '{arg}'" in msg, msg
    assert f"sizes=[{B}, {S}, {HQ}, {D}]" in msg and f"sizes=[{B}, {HQ}, {S}, {D}]" in msg, msg


@pytest.mark.parametrize("arg", ["o", "dout"])
def test_default_rejects_the_bshd_shape(arg):
    shapes = dict(o=(B, HQ, S, D), dout=(B, HQ, S, D))
    shapes[arg] = (B, S, HQ, D)
    msg = _rejected("fa_bwd2", _bwd(**shapes))
    assert f"fa_bwd2: argument '{arg}'" in msg, msg


@pytest.mark.parametrize("arg", ["o", "dout"])
def test_bshd_rejects_a_wrong_dtype(arg):
    msg = _rejected("fa_bwd2", _bwd(**{arg + "_dtype": F32}), bshd=True)
    assert f"fa_bwd2: argument '{arg}'" in msg and "Float" in msg, msg


def test_bshd_refuses_the_fused_kernel():
    args = _bwd()
    args[-1] = True
    msg = _rejected("fa_bwd2", args, bshd=True)
    assert "fused_dvdk=False" in msg, msg
