"""The dense MFMA GEMMs, gemm_tn (five tile geometries) and gemm_tn8 (nine
schedules), against the oracles of tests/gemm_cases.py: exact integer cases
that any fp32 accumulation order must reproduce to the bit, at the K-tile
counts around each pipeline depth, one deep K, and grids of 9, 10 and 15
blocks (two of them not square) for the XCD block remap; a rounding case
with a bound worked out from the arithmetic; and the gemm8-backed linear
against fp64 autograd.  Every shape meets its kernel's divisibility
requirement: no case here can fault the card.  test_gemm_dense.py (CPU)
proves the oracles themselves."""
import pytest
import torch

from tests import gemm_cases as gc

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")


def _ext():
    import vescale_amd.ops as ops

    return ops.require_ext()


def _run_exact(fn, case, tag, bm, bn):
    a, b = case
    got = fn(a.cuda(), b.cuda())
    gc.assert_exact(got, a, b, tag, bm, bn)


# ---------------------------------------------------------------------------
# gemm_tn
# ---------------------------------------------------------------------------
@requires_gpu
@pytest.mark.parametrize("variant", list(gc.TN_VARIANTS))
def test_gemm_tn_pipeline_depths(variant):
    """One tile, K / BK in {1, 2, NBUF-1, NBUF, NBUF+1, 2 NBUF+1} and K =
    4160: the prologue, the counted wait at each K-tile switch and the tail
    take another shape at each."""
    C = _ext()
    bm, bn, bk, _ = gc.TN_VARIANTS[variant]
    for n in gc.tn_ktiles(variant) + [gc.DEEP_K // bk]:
        _run_exact(lambda a, b: C.gemm_tn(a, b, variant), gc.exact_case(bm, bn, n * bk),
                   f"gemm_tn v{variant} {n} K-tiles", bm, bn)


@requires_gpu
@pytest.mark.parametrize("grid", gc.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("variant", list(gc.TN_VARIANTS))
def test_gemm_tn_grids(variant, grid):
    """9, 10 and 15 blocks: the remap branch with q >= 1 and r != 0; on the
    grids that are not square a swap of the two tile coordinates lands
    outside the matrix or in the wrong tile."""
    C = _ext()
    bm, bn, bk, _ = gc.TN_VARIANTS[variant]
    M, N = grid[0] * bm, grid[1] * bn
    k_exact, k_place = gc.grid_ks(bm, bk)
    fn = lambda a, b: C.gemm_tn(a, b, variant)  # noqa: E731
    _run_exact(fn, gc.placement_case(M, N, k_place), f"gemm_tn v{variant} placement {grid}", bm, bn)
    _run_exact(fn, gc.exact_case(M, N, k_exact), f"gemm_tn v{variant} exact {grid}", bm, bn)


# ---------------------------------------------------------------------------
# gemm_tn8
# ---------------------------------------------------------------------------
@requires_gpu
@pytest.mark.parametrize("mode", gc.G8_MODES)
def test_gemm_tn8_tile_counts(mode):
    """One tile at every K / 64 in 1..8 that the mode's guard allows, and
    65 (or 64) tiles: 1, 2 and 3 tiles are the prologue-only, first-wait and
    first-steady-iteration shapes of the rotation schedules."""
    C = _ext()
    for n in gc.g8_ktiles(mode) + [gc.g8_deep_k(mode) // gc.G8_BK]:
        _run_exact(lambda a, b: C.gemm_tn8(a, b, mode),
                   gc.exact_case(gc.G8_BM, gc.G8_BN, n * gc.G8_BK),
                   f"gemm_tn8 mode {mode} {n} K-tiles", gc.G8_BM, gc.G8_BN)


@requires_gpu
@pytest.mark.parametrize("grid", gc.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("mode", gc.G8_MODES)
def test_gemm_tn8_grids(mode, grid):
    C = _ext()
    M, N = grid[0] * gc.G8_BM, grid[1] * gc.G8_BN
    k_exact, k_place = gc.grid_ks(gc.G8_BM, gc.G8_BK, lambda n: gc.g8_ktile_ok(mode, n))
    fn = lambda a, b: C.gemm_tn8(a, b, mode)  # noqa: E731
    _run_exact(fn, gc.placement_case(M, N, k_place), f"gemm_tn8 mode {mode} placement {grid}",
               gc.G8_BM, gc.G8_BN)
    _run_exact(fn, gc.exact_case(M, N, k_exact), f"gemm_tn8 mode {mode} exact {grid}",
               gc.G8_BM, gc.G8_BN)


@requires_gpu
def test_gemm_tn8_guards_reject_before_launch():
    """Mode 5 at 3 K-tiles and modes 7, 8 at 2 are RuntimeErrors, and the
    binding works right after."""
    C = _ext()
    a, b = gc.exact_case(256, 256, 256)
    ad, bd = a.cuda(), b.cuda()
    for mode, k, text in ((5, 192, "mode 5 needs"), (7, 128, "modes 7/8 need"),
                          (8, 128, "modes 7/8 need")):
        with pytest.raises(RuntimeError, match=text):
            C.gemm_tn8(ad[:, :k].contiguous(), bd[:, :k].contiguous(), mode)
        gc.assert_exact(C.gemm_tn8(ad, bd, mode), a, b, f"mode {mode} after the rejection")


@requires_gpu
@pytest.mark.parametrize("mode", gc.G8_FILLED_MODES)
def test_gemm_tn8_filled_machine(mode):
    """256 blocks of 3 K-tiles (4 for the modes that take no odd count): every
    CU starts cold at once, so the loads of the last tile are as late as this
    suite can make them.  Run once per mode: a probe, not a proof.  A wait that
    is too short shows here only if a load happens to be that late; the check
    for the ORDER of waits, issues and reads is the host model of
    test_gemm8_wait_model.py, which walks the schedule tables the kernels are
    built on."""
    C = _ext()
    case = gc.exact_case(gc.FILLED_MN, gc.FILLED_MN, gc.g8_filled_k(mode))
    _run_exact(lambda a, b: C.gemm_tn8(a, b, mode), case, f"gemm_tn8 mode {mode} filled",
               gc.G8_BM, gc.G8_BN)


# ---------------------------------------------------------------------------
# rounding, determinism
# ---------------------------------------------------------------------------
@requires_gpu
@pytest.mark.parametrize("kernel,which", [("gemm_tn8", 0), ("gemm_tn8", 4), ("gemm_tn", 0),
                                          ("gemm_tn", 1), ("gemm_tn", 4)])
def test_rounding_case(kernel, which):
    C = _ext()
    M, N, K = gc.ROUNDING_SHAPE
    a, b = gc.rounding_case(M, N, K)
    got = getattr(C, kernel)(a.cuda(), b.cuda(), which)
    gc.assert_within_rounding(got, a, b, f"{kernel} {which} {M}x{N}x{K}")


@requires_gpu
@pytest.mark.parametrize("kernel,which", [("gemm_tn", 0), ("gemm_tn", 1), ("gemm_tn", 3),
                                          ("gemm_tn", 4), ("gemm_tn8", 0), ("gemm_tn8", 4),
                                          ("gemm_tn8", 6), ("gemm_tn8", 7), ("gemm_tn8", 8)])
def test_two_calls_give_equal_bits(kernel, which):
    """One shape per schedule family, two calls on the same operands."""
    C = _ext()
    a, b = gc.rounding_case(1024, 768, 1088 if kernel == "gemm_tn" else 1024)
    ad, bd = a.cuda(), b.cuda()
    first = getattr(C, kernel)(ad, bd, which)
    second = getattr(C, kernel)(ad, bd, which)
    assert torch.equal(first.view(torch.int16), second.view(torch.int16))


# ---------------------------------------------------------------------------
# _Linear8 and linear() under VESCALE_GEMM=gemm8
# ---------------------------------------------------------------------------
@requires_gpu
@pytest.mark.parametrize("entry", ["_Linear8", "linear"])
@pytest.mark.parametrize("name", list(gc.LINEAR8_CASES))
def test_linear_gemm8_against_fp64_autograd(name, entry, monkeypatch):
    """y, dx and dw against fp64 autograd, each within the rounding bound of
    the GEMM that makes it, whether the in-tree kernel or the library runs it."""
    from vescale_amd.ops import functional as F

    x_cpu, w_cpu, dy_cpu = gc.linear8_case(name)
    (y_ref, dx_ref, dw_ref), bounds = gc.linear8_oracle(x_cpu, w_cpu, dy_cpu)
    if gc.LINEAR8_CASES[name][2] == "strided":
        wide = torch.zeros(x_cpu.shape[0], 2 * x_cpu.shape[1], dtype=torch.bfloat16, device="cuda")
        wide[:, ::2] = x_cpu.cuda()
        x = wide[:, ::2]
        assert not x.is_contiguous()
    else:
        x = x_cpu.cuda()
    x.requires_grad_()
    w = w_cpu.cuda().requires_grad_()
    if entry == "linear":
        monkeypatch.setenv("VESCALE_GEMM", "gemm8")
        y = F.linear(x, w)
    else:
        y = F._Linear8.apply(x, w)
    y.backward(dy_cpu.cuda())
    assert x.grad.shape == x.shape
    for what, got, ref, bound in (("y", y.detach(), y_ref, bounds[0]),
                                  ("dx", x.grad, dx_ref, bounds[1]),
                                  ("dw", w.grad, dw_ref, bounds[2])):
        err = (got.cpu().double() - ref).abs()
        print(f"{name} {entry} {what}: max |err| / bound = "
              f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert got.shape == ref.shape and bool((err <= bound).all()), (name, entry, what)
