"""Binding contract of the vocab-parallel forms of ce_fwd / ce_bwd (trailing
keywords vocab_start, vocab_total), exercised WITHOUT a device like
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

BF, F32, I64 = torch.bfloat16, torch.float32, torch.int64


def T(*shape, dtype=BF):
    # uninitialised on purpose, see test_ext_contract.T
    return torch.empty(*shape, dtype=dtype)


def _args(name, n=64):
    if name == "ce_fwd":
        return [T(2, n), T(2, dtype=I64), -100]
    return [T(2, n), T(2, dtype=I64), T(2, dtype=F32), T(2, dtype=F32), -100, False]


def _rejected(name, args, **kw):
    with pytest.raises(RuntimeError) as ei:
        getattr(ops._C, name)(*args, **kw)
    msg = str(ei.value)
    assert "ROCm-capable" not in msg and "HIP error" not in msg, msg
    return msg


@pytest.mark.parametrize("name", ["ce_fwd", "ce_bwd"])
def test_keyword_form_is_rejected_before_the_device(name):
    msg = _rejected(name, _args(name), vocab_start=64, vocab_total=256)
    assert f"{name}: argument 'logits'" in msg and "cpu" in msg, msg
    # the dense default spelled out is the same call as today's
    msg = _rejected(name, _args(name), vocab_start=0, vocab_total=-1)
    assert f"{name}: argument 'logits'" in msg and "cpu" in msg, msg


@pytest.mark.parametrize("name", ["ce_fwd", "ce_bwd"])
@pytest.mark.parametrize("n,kw,fact", [
    (64, dict(vocab_start=-1, vocab_total=256), "vocab_start = -1"),
    (64, dict(vocab_start=200, vocab_total=256), "vocab_start + n = 200 + 64 is past vocab_total = 256"),
    (64, dict(vocab_start=0, vocab_total=63), "is past vocab_total = 63"),
    (64, dict(vocab_start=0, vocab_total=-2), "vocab_total = -2"),
    (64, dict(vocab_start=8, vocab_total=-1), "vocab_start + n = 8 + 64"),
    (60, dict(vocab_start=0, vocab_total=240), "= 60 must be a positive multiple of 8"),
])
def test_scalar_rule(name, n, kw, fact):
    msg = _rejected(name, _args(name, n), **kw)
    assert name in msg and fact in msg, msg


@pytest.mark.parametrize("name,pos,arg", [
    ("ce_fwd", 1, "target"), ("ce_bwd", 1, "target"), ("ce_bwd", 2, "lse"), ("ce_bwd", 3, "dloss"),
])
def test_keyword_form_names_a_bad_argument(name, pos, arg):
    args = _args(name)
    args[pos] = T(3, dtype=args[pos].dtype)
    msg = _rejected(name, args, vocab_start=64, vocab_total=256)
    assert f"{name}: argument '{arg}'" in msg and "sizes=[3]" in msg, msg
