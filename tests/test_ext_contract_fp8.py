"""Binding contract of the fp8 forms of gemm_tn8 (the fp8 GEMM, fp8_amax,
fp8_quantize), exercised WITHOUT a device like test_ext_contract_grouped.py:
every call ends in a RuntimeError of host validation."""
import pytest
import torch

import vescale_amd.ops as ops

pytestmark = [
    pytest.mark.skipif(not ops.has_ext(), reason="needs the built extension"),
    pytest.mark.skipif(torch.cuda.is_available(),
                       reason="CPU-only: with a GPU a missed check reaches a kernel"),
]

BF, F32, E4M3, E5M2 = torch.bfloat16, torch.float32, torch.float8_e4m3fn, torch.float8_e5m2
GPU_ONLY = "gemm_tn8: argument 'a' expected device=a GPU; got device=cpu"


def T(*shape, dtype=BF):
    # uninitialised on purpose, see test_ext_contract.T
    return torch.empty(*shape, dtype=dtype)


def _gemm(m=256, n=256, k=128, mode=0, bdt=E4M3, **over):
    kw = dict(scale_a=T(1, dtype=F32), scale_b=T(1, dtype=F32))
    kw.update(over)
    return (T(m, k, dtype=E5M2), T(n, k, dtype=bdt), mode), kw


def _quant(r=64, c=128, **over):
    kw = dict(group_form="fp8_quantize", scale_a=T(1, dtype=F32),
              group_out=T(r, c, dtype=E4M3), out_t=T(c, r, dtype=E4M3))
    kw.update(over)
    return (T(r, c), [], 0), kw


@pytest.mark.parametrize("call,fact", [
    (_gemm(), GPU_ONLY),  # all valid: only the device is wrong
    (_quant(), GPU_ONLY),
    (((T(64, 64), [], 0), dict(group_form="fp8_amax")), GPU_ONLY),
    (_gemm(scale_a=None), "argument 'scale_a' expected"),
    (_gemm(scale_b=T(1, dtype=torch.float64)), "argument 'scale_b' expected"),
    (_gemm(scale_b=T(2, dtype=F32)), "argument 'scale_b' expected"),
    (_gemm(bdt=E5M2), "argument 'b' expected"),
    (_gemm(k=192), "K % 128 == 0"),
    (_gemm(m=128), "M % 256 == 0"),
    (_gemm(mode=1), "mode = 1 must be 0 with fp8 operands"),
    (_gemm(group_form="fp8"), "group_form = 'fp8' must be"),
    (_quant(group_out=None, out_t=None), "needs group_out, out_t or both"),
    (_quant(out_t=T(128, 64, dtype=E5M2)), "argument 'out_t' expected"),
    (_quant(out_t=T(64, 128, dtype=E4M3)), "argument 'out_t' expected"),
    (_quant(r=32), "R % 64 == 0"),
])
def test_rejected_before_the_device(call, fact):
    args, kw = call
    with pytest.raises(RuntimeError) as ei:
        ops._C.gemm_tn8(*args, **kw)
    msg = str(ei.value)
    assert "ROCm-capable" not in msg and "HIP error" not in msg, msg
    assert "gemm_tn8" in msg and fact in msg, msg
