"""Binding contract of the grouped forms of gemm_tn8, exercised WITHOUT a device
like test_ext_contract.py: every call ends in a RuntimeError of host validation."""
import pytest
import torch

import vescale_amd.ops as ops

pytestmark = [
    pytest.mark.skipif(not ops.has_ext(), reason="needs the built extension"),
    pytest.mark.skipif(torch.cuda.is_available(),
                       reason="CPU-only: with a GPU a missed check reaches a kernel"),
]

BF, I32 = torch.bfloat16, torch.int32
T_ROWS, N, K, E = 8, 256, 128, 4


def T(*shape, dtype=BF):
    # uninitialised on purpose, see test_ext_contract.T
    return torch.empty(*shape, dtype=dtype)


def _call(form, *, n=N, k=K, e=E, b=None, **over):
    kw = dict(group_offsets=T(e + 1, dtype=I32), group_form=form)
    if form == "wgrad":
        kw["group_x"] = T(T_ROWS, k)
    kw.update(over)
    a = T(T_ROWS, k if form == "fwd" else n)
    return a, (b if b is not None else [T(n, k) for _ in range(e)]), kw


def _rejected(a, b, kw):
    with pytest.raises(RuntimeError) as ei:
        ops._C.gemm_tn8(a, b, 0, **kw)
    msg = str(ei.value)
    assert "ROCm-capable" not in msg and "HIP error" not in msg, msg
    return msg


@pytest.mark.parametrize("form", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("over,fact", [
    (dict(), "gemm_tn8: argument 'a' expected device=a GPU; got device=cpu"),  # all else valid
    (dict(b=T(E, N, K)), "gemm_tn8: argument 'a' expected device=a GPU; got device=cpu"),
    (dict(k=192), "K = 192 must be a positive multiple of 128"),
    (dict(n=64), "N = 64 must be a positive multiple of 128"),
    (dict(e=65), "E = 65 experts must be in 1..64"),
    (dict(e=0), "E = 0 experts must be in 1..64"),
    (dict(group_form="bwd"), "group_form = 'bwd' must be 'fwd', 'dgrad' or 'wgrad'"),
    (dict(group_offsets=None), "needs group_offsets"),
    (dict(group_offsets=T(E + 1, dtype=torch.int64)), "argument 'group_offsets' expected"),
    (dict(group_offsets=T(E, dtype=I32)), "argument 'group_offsets' expected"),
    (dict(b=[T(N, K), T(N, K), T(K, N), T(N, K)]), "argument 'b[2]' expected"),
    (dict(b=T(N, K)), "one [E,N,K] tensor"),
    (dict(group_out=T(3, 3)), "argument 'group_out' expected"),
    (dict(group_x=T(T_ROWS + 1, K)), "group_x"),
])
def test_rejected_before_the_device(form, over, fact):
    msg = _rejected(*_call(form, **over))
    assert "gemm_tn8" in msg and fact in msg, msg

