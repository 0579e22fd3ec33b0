"""fa_bwd2 refuses a softmax scale that is not positive and finite, without a
device: its kernels write -inf into the masked scores before they scale them,
which stays -inf only under such a scale.  (Conditions as in
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

BF, F32 = torch.bfloat16, torch.float32


def _args(scale):
    T = torch.empty
    return [T(1, 2, 256, 128, dtype=BF), T(1, 1, 256, 128, dtype=BF), T(1, 1, 256, 128, dtype=BF),
            T(1, 2, 256, 128, dtype=BF), T(1, 2, 256, 128, dtype=BF), T(1, 2, 256, dtype=F32),
            scale, False]


@pytest.mark.parametrize("scale", [0.0, -0.125, float("inf"), float("nan")])
def test_fa_bwd2_refuses_the_scale(scale):
    with pytest.raises(RuntimeError) as ei:
        ops._C.fa_bwd2(*_args(scale))
    msg = str(ei.value)
    assert "fa_bwd2: scale" in msg and "positive and finite" in msg, msg
    assert "ROCm-capable" not in msg and "HIP error" not in msg, msg
