"""Binding contract of the relayout probe (_relayout_probe), without a device.

It is the one probe that takes an argument, so unlike the argument-less probes
it goes through the launch layer's argument check: on a CPU-only box every
call must end in that check's RuntimeError, naming the argument, and never in
a HIP runtime error.  (Conditions as in test_ext_contract.py.)
"""
import pytest
import torch

import vescale_amd.ops as ops

pytestmark = [
    pytest.mark.skipif(not ops.has_ext(), reason="needs the built extension"),
    pytest.mark.skipif(torch.cuda.is_available(),
                       reason="CPU-only: with a GPU a missed check reaches a kernel"),
]


def _rejected(x):
    with pytest.raises(RuntimeError) as ei:
        ops._C._relayout_probe(x)
    msg = str(ei.value)
    assert "ROCm-capable" not in msg and "HIP error" not in msg, msg
    return msg


def test_valid_cpu_call_is_rejected_before_the_device():
    msg = _rejected(torch.empty(64, 32, dtype=torch.float32))
    assert "_relayout_probe: argument 'x'" in msg and "cpu" in msg, msg


@pytest.mark.parametrize("x", [
    torch.empty(64, 32, dtype=torch.bfloat16),
    torch.empty(64, 33, dtype=torch.float32),
    torch.empty(32, 32, dtype=torch.float32),
    torch.empty(64, 64, dtype=torch.float32)[:, ::2],
], ids=["dtype", "wide", "short", "strided"])
def test_one_bad_argument_is_named(x):
    msg = _rejected(x)
    assert "_relayout_probe: argument 'x' expected" in msg, msg
