"""rmsnorm_bwd over the instantiations its binding selects by hidden (8-element
chunks per thread: hidden 8 and 520 run 1, 4096 runs 2, 6144 runs 3, 8192 runs 4; most
threads idle at 8 and 520); 1, 3 and 33 rows are fewer blocks than the grid
cap, 2051 rows make the 1024 blocks loop; with and without the fused residual
gradient.

dx against an fp64 reference at test_rmsnorm_fwd_bwd's tolerances; dw with
the bound of test_rmsnorm_bwd_dw_repeatable; dx and dw bitwise repeatable."""
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

EPS = 1e-5


@requires_gpu
@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("hidden", [8, 520, 4096, 6144, 8192])
@pytest.mark.parametrize("rows", [1, 3, 33, 2051])
def test_rmsnorm_bwd_shapes(rows, hidden, with_dres):
    import vescale_amd.ops as ops

    C = ops.require_ext()
    torch.manual_seed(rows * 10007 + hidden)
    x = torch.randn(rows, hidden, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(hidden, device="cuda", dtype=torch.bfloat16)
    dy = torch.randn(rows, hidden, device="cuda", dtype=torch.bfloat16)
    dres = torch.randn(rows, hidden, device="cuda", dtype=torch.bfloat16) if with_dres else None
    # the rrms the forward kernel saves for the backward
    _, rrms = C.rmsnorm_fwd(x, w, EPS)

    dx0, dw0 = C.rmsnorm_bwd(dy, x, w, rrms, dres)
    assert dx0.shape == x.shape and dx0.dtype == torch.bfloat16
    assert dw0.shape == (hidden,) and dw0.dtype == torch.float32
    for _ in range(3):
        dx, dw = C.rmsnorm_bwd(dy, x, w, rrms, dres)
        assert torch.equal(dx, dx0), "dx is not bitwise repeatable"
        assert torch.equal(dw, dw0), "dw is not bitwise repeatable"

    xd, dyd, wd = x.double(), dy.double(), w.double()
    r = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + EPS)
    dot = (dyd * wd * xd).sum(-1, keepdim=True)
    dx_ref = r * wd * dyd - xd * dot * r.pow(3) / hidden
    if with_dres:
        dx_ref = dx_ref + dres.double()
    dx_err = (dx0.double() - dx_ref).abs()
    print(f"dx max err {float(dx_err.max()):.3e}")
    assert torch.allclose(dx0.double(), dx_ref, atol=5e-2, rtol=5e-2), float(dx_err.max())

    terms = dyd * xd * r
    ref, abs_sum = terms.sum(0), terms.abs().sum(0)
    # the binding returns fp32 dw; the wrappers round it to bf16 (the 2^-8 term)
    err = (dw0.to(torch.bfloat16).double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + (rows + 32) * 2.0 ** -24 * abs_sum
    print(f"dw max err {float(err.max()):.3e}, max (err - bound) {float((err - bound).max()):.3e}")
    assert bool((err <= bound).all()), float((err - bound).max())
