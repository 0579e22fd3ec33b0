"""The dense wgrad layout path without a device: ops.linear falls back to
F.linear exactly, and the host validation of the two new binding forms names
what is wrong before anything could launch."""
import pytest
import torch

import vescale_amd.ops as ops
from vescale_amd.ops import functional as VF

needs_ext = pytest.mark.skipif(not ops.has_ext(), reason="needs the built extension")
BF = torch.bfloat16


def T(*shape):
    return torch.empty(*shape, dtype=BF)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("form", [None, "c"])
def test_cpu_linear_is_f_linear(dtype, form):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 16, generator=g).to(dtype)
    w = torch.randn(24, 16, generator=g).to(dtype)
    dy = torch.randn(2, 8, 24, generator=g).to(dtype)
    got, want = [], []
    for fn, out in ((lambda a, b: VF.linear(a, b, _wgrad_form_override=form), got),
                    (torch.nn.functional.linear, want)):
        xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = fn(xg, wg)
        out.extend([y.detach(), *torch.autograd.grad(y, (xg, wg), dy)])
    assert "LinearWgrad" not in type(VF.linear(x.requires_grad_(), w).grad_fn).__name__
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_static_rule_is_a_pure_function_of_the_shape():
    for m, n, k in [(32768, 6144, 4096), (32768, 4096, 4096), (32768, 28672, 4096),
                    (32768, 4096, 14336), (32768, 128256, 4096), (256, 64, 128)]:
        form = VF._wgrad_form(m, n, k)
        assert form in VF.WGRAD_FORMS and form == VF._wgrad_form(m, n, k)


def _rejected(fn, *args, **kw):
    with pytest.raises(RuntimeError) as ei:
        fn(*args, **kw)
    msg = str(ei.value)
    assert "ROCm-capable" not in msg and "HIP error" not in msg, msg
    return msg


@needs_ext
@pytest.mark.parametrize("shape", [(12, 8), (8, 12), (7, 64), (64, 63)])
def test_transpose_refuses_extents_that_are_no_multiple_of_8(shape):
    msg = _rejected(ops._C.gemm_tn8, T(*shape), [], 0, group_form="transpose")
    assert "gemm_tn8: argument 'a'" in msg and "% 8 == 0" in msg and str(list(shape)) in msg


@needs_ext
def test_transpose_scalar_and_operand_rules():
    f = ops._C.gemm_tn8
    assert "b must be []" in _rejected(f, T(8, 8), T(8, 8), 0, group_form="transpose")
    assert "b must be []" in _rejected(f, T(8, 8), [T(8, 8)], 0, group_form="transpose")
    assert "mode 0 or 1" in _rejected(f, T(8, 8), [], 2, group_form="transpose")
    assert "must be [R,C]" in _rejected(f, T(2, 8, 8), [], 0, group_form="transpose")
    # a well-formed call made of CPU tensors ends at the device check
    msg = _rejected(f, T(8, 8), [], 0, group_form="transpose")
    assert "gemm_tn8: argument 'a'" in msg and "cpu" in msg
    msg = _rejected(f, torch.empty(8, 8, dtype=torch.float64), [], 0, group_form="transpose")
    assert "gemm_tn8: argument 'a'" in msg and "dtype=Double" in msg
    msg = _rejected(f, T(8, 8, 2)[..., 0], [], 0, group_form="transpose")
    assert "gemm_tn8: argument 'a'" in msg and "contiguous=false" in msg


@needs_ext
def test_swiglu_transposed_validation():
    f = ops._C.swiglu_packed_bwd
    msg = _rejected(f, T(4, 16), T(4, 32), transposed=True)
    assert "swiglu_packed_bwd" in msg and "rows" in msg and "multiple of 8" in msg
    for kw in ({}, {"transposed": True}):
        msg = _rejected(f, T(8, 16), T(8, 32), **kw)
        assert "swiglu_packed_bwd: argument 'dy'" in msg and "cpu" in msg
        msg = _rejected(f, T(8, 17), T(8, 32), **kw)
        assert "swiglu_packed_bwd: argument 'dy'" in msg and "sizes=[8, 17]" in msg
