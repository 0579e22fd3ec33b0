"""Binding contract of the keywords causal (fa_fwd, fa_bwd2) and dlse (fa_bwd2),
WITHOUT a device like test_ext_contract_segments.py: every call must end in a
RuntimeError raised by host validation, never in a HIP runtime error."""
import pytest
import torch

import vescale_amd.ops as ops

pytestmark = [
    pytest.mark.skipif(not ops.has_ext(), reason="needs the built extension"),
    pytest.mark.skipif(torch.cuda.is_available(),
                       reason="CPU-only: with a GPU a missed check reaches a kernel"),
]

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
B, HQ, HKV, SQ, SK, D = 1, 2, 1, 256, 512, 128


def T(*shape, dtype=BF):  # uninitialised on purpose, see test_ext_contract.T
    return torch.empty(*shape, dtype=dtype)


def _rejected(name, sk, sv=None, fused_dvdk=False, **kw):
    args = [T(B, HQ, SQ, D), T(B, HKV, sk, D), T(B, HKV, sv or sk, D)]
    if name == "fa_bwd2":
        args += [T(B, HQ, SQ, D), T(B, HQ, SQ, D), T(B, HQ, SQ, dtype=F32)]
        kw["fused_dvdk"] = fused_dvdk
    with pytest.raises(RuntimeError) as ei:
        getattr(ops._C, name)(*args, 0.1, **kw)
    msg = str(ei.value)
    assert "ROCm-capable" not in msg and "HIP error" not in msg, msg
    return msg


DLSE, BOUNDS = T(B, HQ, SQ, dtype=F32), T(B, 2, SQ, dtype=I32)


SIZES = " expected device=cpu (must be a GPU) dtype=BFloat16 sizes=[%d, %d, %d, %d]"
NO_GPU = ": argument 'q' expected device=a GPU; got device=cpu"   # valid: the launch refuses


@pytest.mark.parametrize("name,sk,sv,kw,fact", [
    (n, *c) for n in ("fa_fwd", "fa_bwd2") for c in [
        (SK, None, dict(causal=False), NO_GPU),
        (SQ, None, dict(causal=True), NO_GPU),
        (128, None, dict(causal=False), ": with causal=False the k/v seq = 128 must be a positive multiple of 256"),
        (SK, SQ, dict(causal=False), ": argument 'v'" + SIZES % (B, HKV, SK, D)),
        # the default keeps the square contract: k is named
        (SK, None, dict(), ": argument 'k'" + SIZES % (B, HKV, SQ, D)),
    ]] + [
    ("fa_bwd2", SK, None, dict(causal=False, dlse=DLSE), NO_GPU),
    ("fa_bwd2", SQ, None, dict(dlse=DLSE, seg_bounds=BOUNDS), NO_GPU),
    ("fa_fwd", SK, None, dict(causal=False, segment_ids=T(B, SQ, dtype=I32)), ": causal=False takes no segment_ids"),
    ("fa_bwd2", SK, None, dict(causal=False, seg_bounds=BOUNDS), ": causal=False takes no seg_bounds"),
    ("fa_bwd2", SK, None, dict(causal=False, fused_dvdk=True), ": the fused dv+dk kernel is causal"),
])
def test_keyword_forms(name, sk, sv, kw, fact):
    assert name + fact in _rejected(name, sk, sv, **kw)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dlse,fact", [
    (T(B, HQ, SQ, dtype=BF), "dtype=BFloat16 "),
    (T(B, HQ, SQ + 1, dtype=F32), f"sizes=[{B}, {HQ}, {SQ + 1}] "),
    (T(B, HQ, SK, dtype=F32), f"sizes=[{B}, {HQ}, {SK}] "),       # k's length is not q's
    (T(B, HQ, SQ, 2, dtype=F32)[..., 0], "contiguous=false"),
])
def test_one_bad_dlse_is_named(causal, dlse, fact):
    msg = _rejected("fa_bwd2", SQ if causal else SK, causal=causal, dlse=dlse)
    assert "fa_bwd2: argument 'dlse'" in msg, msg
    assert fact in msg[msg.index("; got "):], msg
