"""Binding contract of the staging probe (_stage_probe), without a device.

Like _relayout_probe it takes arguments, so it goes through the launch layer's
argument check: on a CPU-only box every call must end in a RuntimeError that
names what is wrong, and never in a HIP runtime error.  (Conditions as in
test_ext_contract.py.)
"""
import pytest
import torch

import vescale_amd.ops as ops

pytestmark = [
    pytest.mark.skipif(not ops.has_ext(), reason="needs the built extension"),
    pytest.mark.skipif(torch.cuda.is_available(),
                       reason="CPU-only: with a GPU a missed check reaches a kernel"),
]


def _rejected(x, threads):
    with pytest.raises(RuntimeError) as ei:
        ops._C._stage_probe(x, threads)
    msg = str(ei.value)
    assert "ROCm-capable" not in msg and "HIP error" not in msg, msg
    return msg


def test_valid_cpu_call_is_rejected_before_the_device():
    msg = _rejected(torch.empty(64, 128, dtype=torch.bfloat16), 256)
    assert "_stage_probe: argument 'x'" in msg and "cpu" in msg, msg


@pytest.mark.parametrize("x", [
    torch.empty(64, 128, dtype=torch.float32),
    torch.empty(64, 128, 1, dtype=torch.bfloat16),
    torch.empty(64, 256, dtype=torch.bfloat16)[:, ::2],
], ids=["dtype", "rank", "strided"])
def test_one_bad_argument_is_named(x):
    msg = _rejected(x, 256)
    assert "_stage_probe: argument 'x' expected" in msg, msg


@pytest.mark.parametrize("x,threads,what", [
    (torch.empty(128, 128, dtype=torch.bfloat16), 256, "rows = 128"),
    (torch.empty(64, 192, dtype=torch.bfloat16), 256, "stride = 192"),
    (torch.empty(64, 64, dtype=torch.bfloat16), 256, "stride = 64"),
    (torch.empty(64, 128, dtype=torch.bfloat16), 128, "threads = 128"),
], ids=["rows", "stride", "narrow", "threads"])
def test_one_bad_scalar_is_named(x, threads, what):
    msg = _rejected(x, threads)
    assert "_stage_probe: " + what in msg, msg
