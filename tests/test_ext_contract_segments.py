"""Binding contract of the segment-masked forms of fa_gen_fwd / fa_gen_bwd
(trailing keywords q_seg, kv_seg), exercised WITHOUT a device like
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

BF, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
B, HQ, HKV, SQ, SK, D = 2, 2, 1, 8, 12, 64
NAMES = ["fa_gen_fwd", "fa_gen_bwd"]


def T(*shape, dtype=BF):
    # uninitialised on purpose, see test_ext_contract.T
    return torch.empty(*shape, dtype=dtype)


def _args(name):
    qkv = [T(B, HQ, SQ, D), T(B, HKV, SK, D), T(B, HKV, SK, D)]
    if name == "fa_gen_fwd":
        return qkv + [0.1, True, 0]
    return qkv + [T(B, HQ, SQ, D), T(B, HQ, SQ, D), T(B, HQ, SQ, dtype=F32),
                  T(B, HQ, SQ, dtype=F32), 0.1, True, 0]


def _seg(q=(B, SQ), kv=(B, SK), q_dtype=I32, kv_dtype=I32):
    return dict(q_seg=T(*q, dtype=q_dtype), kv_seg=T(*kv, dtype=kv_dtype))


def _rejected(name, args, **kw):
    with pytest.raises(RuntimeError) as ei:
        getattr(ops._C, name)(*args, **kw)
    msg = str(ei.value)
    assert "ROCm-capable" not in msg and "HIP error" not in msg, msg
    return msg


@pytest.mark.parametrize("name", NAMES)
def test_keyword_form_is_rejected_before_the_device(name):
    msg = _rejected(name, _args(name), **_seg())
    assert f"{name}: argument 'q'" in msg and "cpu" in msg, msg
    # the default spelled out is the same call as today's
    msg = _rejected(name, _args(name), q_seg=None, kv_seg=None)
    assert f"{name}: argument 'q'" in msg and "cpu" in msg, msg


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("given", ["q_seg", "kv_seg"])
def test_one_segment_tensor_without_the_other(name, given):
    msg = _rejected(name, _args(name), **{given: _seg()[given]})
    assert f"{name}: q_seg and kv_seg must be given together" in msg, msg


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("arg,kw,fact", [
    ("q_seg", dict(q_dtype=I64), "dtype=Long "),
    ("kv_seg", dict(kv_dtype=I64), "dtype=Long "),
    ("q_seg", dict(q=(B, SQ + 1)), f"sizes=[{B}, {SQ + 1}] "),
    ("q_seg", dict(q=(B + 1, SQ)), f"sizes=[{B + 1}, {SQ}] "),
    ("kv_seg", dict(kv=(B, SK + 1)), f"sizes=[{B}, {SK + 1}] "),
    ("kv_seg", dict(kv=(B + 1, SK)), f"sizes=[{B + 1}, {SK}] "),
    ("kv_seg", dict(kv=(B, SQ)), f"sizes=[{B}, {SQ}] "),      # q's shape is not kv's
    ("q_seg", dict(q=(B * SQ,)), f"sizes=[{B * SQ}] "),
])
def test_one_bad_segment_argument_is_named(name, arg, kw, fact):
    msg = _rejected(name, _args(name), **_seg(**kw))
    assert f"{name}: argument '{arg}'" in msg, msg
    assert fact in msg[msg.index("; got "):], msg


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("arg", ["q_seg", "kv_seg"])
def test_strided_segment_argument_is_named(name, arg):
    kw = _seg()
    t = kw[arg]
    kw[arg] = T(*t.shape, 2, dtype=I32)[..., 0]
    assert kw[arg].shape == t.shape and not kw[arg].is_contiguous()
    msg = _rejected(name, _args(name), **kw)
    assert f"{name}: argument '{arg}'" in msg and "contiguous=false" in msg, msg
