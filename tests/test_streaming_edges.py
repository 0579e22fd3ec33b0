"""CPU tier of the streaming-kernel edge tests: the fp64 oracles and the numpy
Philox4x32-10 of tests/streaming_cases.py are verified here without a GPU -
the oracles against the torch fallbacks of ops/functional.py at the cases the
GPU tier (test_streaming_edges_gpu.py, test_philox_reference_gpu.py) runs the
HIP kernels at, the Philox reference against the Random123 known answers, and
the stream-independence caps against streams that are independent by
construction.  Tolerances are the GPU tier's; their sources are named there.
"""
import numpy as np
import pytest
import torch

from tests import streaming_cases as sc
from tests.vp_ce_cases import GRAD_TOL, IGNORE, LOSS_TOL, oracle


# ---------------------------------------------------------------------------
# Philox
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(counter, key, want):
    got = tuple(int(w) for w in sc.philox4x32_10(counter, key))
    assert got == want, [hex(w) for w in got]
    # the same through the vectorised path
    arr = sc.philox4x32_10(tuple(np.full(3, c, dtype=np.uint32) for c in counter), key)
    assert all((a == w).all() for a, w in zip(arr, want))


def test_philox_kernel_layout():
    seed, g = (1 << 40) + 7, np.arange(64)
    w = sc.kernel_words(seed, (1 << 32) - 1, g, 1)
    assert w.shape == (64, 4) and w.dtype == np.uint32
    # elements 4..7 share the counter (0, 1, stream, 0): the offset carried
    direct = sc.philox4x32_10((0, 1, 1, 0), (7, 1 << 8))
    assert [int(x) for x in w[5]] == [int(x) for x in direct]
    # one unit of offset is one counter, four elements
    assert (sc.kernel_words(seed, 3, g, 0) == sc.kernel_words(seed, 0, g + 12, 0)).all()
    u = sc.ref_uniform(seed, 0, np.arange(1 << 16))
    assert u.dtype == np.float32 and u.min() > 0.0 and u.max() <= 1.0
    assert sc.word_to_uniform(np.array([0, 0xFFFFFFFF], dtype=np.uint32)).tolist() == [2.0 ** -32, 1.0]
    idx = sc.shard_global_index([5, 6, 7], [2, 3, 4], [1, 2, 3])
    full = np.arange(5 * 6 * 7).reshape(5, 6, 7)
    assert (idx == full[1:3, 2:5, 3:7].reshape(-1)).all()


def test_independent_streams_pass_the_lag_caps():
    """Two [256, 256] ops at disjoint counter ranges of one seed (offsets 0
    and numel / 4) satisfy the caps that test_philox_reference_gpu.py puts on
    two consecutive ops; two ops 4 counters apart (16 elements) break both."""
    n, seed = 256 * 256, 777
    g = np.arange(n)
    u = [sc.ref_uniform(seed, off, g) for off in (0, n // 4, 4)]
    assert sc.mask_agreement_violations(u[0] > 0.5, u[1] > 0.5) == []
    assert (16, 1.0) in sc.mask_agreement_violations(u[0] > 0.5, u[2] > 0.5)
    z = [sc.ref_normal64(seed, off, g).astype(np.float32) for off in (0, n // 4, 4)]
    assert np.isfinite(z[0]).all() and np.abs(z[0]).max() <= 6.67
    assert abs(z[0].mean()) < 0.02 and abs(z[0].std() - 1) < 0.02
    assert sc.max_equal_values(z[0], z[1])[0] <= 2
    assert sc.max_equal_values(z[0], z[2]) == (n - 16, 16)


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------
def _swiglu_fallback(g, u, dy):
    from vescale_amd.ops import swiglu

    g, u = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
    out = swiglu(g, u)
    out.backward(dy)
    return out.detach(), g.grad, u.grad


def _swiglu_packed_fallback(gu, dy):
    from vescale_amd.ops import swiglu_packed

    gu = gu.clone().requires_grad_(True)
    out = swiglu_packed(gu)
    out.backward(dy)
    return out.detach(), gu.grad


@pytest.mark.parametrize("n", sc.FLAT_SIZES)
def test_swiglu_oracle(n):
    g, u, dy = sc.swiglu_case(n)
    out, dg, du = _swiglu_fallback(g, u, dy)
    r_out, r_dg, r_du = sc.swiglu_oracle(g, u, dy)
    assert torch.allclose(out.double(), r_out, **sc.SWIGLU_OUT_TOL)
    assert torch.allclose(dg.double(), r_dg, **sc.SWIGLU_GRAD_TOL)
    assert torch.allclose(du.double(), r_du, **sc.SWIGLU_GRAD_TOL)


@pytest.mark.parametrize("rows,F2", sc.SWIGLU_PACKED_SHAPES)
def test_swiglu_packed_oracle(rows, F2):
    gu, dy = sc.swiglu_packed_case(rows, F2)
    F = F2 // 2
    out, dgu = _swiglu_packed_fallback(gu, dy)
    r_out, r_dg, r_du = sc.swiglu_oracle(gu[:, :F], gu[:, F:], dy)
    assert torch.allclose(out.double(), r_out, **sc.SWIGLU_OUT_TOL)
    assert torch.allclose(dgu.double(), torch.cat([r_dg, r_du], -1), **sc.SWIGLU_GRAD_TOL)
    sep = _swiglu_fallback(gu[:, :F].contiguous(), gu[:, F:].contiguous(), dy)
    assert sc.same_bits(out, sep[0]) and sc.same_bits(dgu, torch.cat(sep[1:], -1))


def test_swiglu_special_values_oracle():
    g, u, dy = sc.swiglu_special_case()
    assert g.isfinite().all() and g.abs().max() > 2.9e38 and (g == 0).sum() == 30
    refs = sc.swiglu_oracle(g, u, dy)
    assert not any(r.isnan().any() for r in refs)
    assert refs[0].bfloat16().isinf().any() and refs[2].bfloat16().isinf().any()
    for got, ref in zip(_swiglu_fallback(g, u, dy), refs):
        assert sc.same_nonfinite(got, ref)


# ---------------------------------------------------------------------------
# dense cross-entropy
# ---------------------------------------------------------------------------
def _ce_fallback(x, target, g_rows):
    from vescale_amd.ops import fused_cross_entropy, vocab_parallel_cross_entropy

    a = x.clone().requires_grad_(True)
    mean = fused_cross_entropy(a, target, IGNORE)
    mean.backward()
    b = x.clone().requires_grad_(True)
    rows = vocab_parallel_cross_entropy(b, target, 0, x.shape[1], ignore_index=IGNORE,
                                        reduction="none")
    rows.backward(g_rows)
    return dict(mean=(mean.detach(), a.grad), none=(rows.detach(), b.grad))


@pytest.mark.parametrize("V,N", sc.CE_SHAPES)
def test_ce_oracle(V, N):
    x, target, g_rows = sc.ce_case(V, N)
    assert (target == IGNORE).sum() == 2 and x[3].min() > 9000 and x[4].max() < -9000
    got = _ce_fallback(x, target, g_rows)
    for reduction in ("mean", "none"):
        ref_loss, ref_grad = oracle(x.double(), target, reduction, g_rows)
        loss, grad = got[reduction]
        assert torch.allclose(loss.double(), ref_loss, **LOSS_TOL)
        assert torch.allclose(grad.double(), ref_grad, **GRAD_TOL)
        assert not grad[target == IGNORE].any()


@pytest.mark.parametrize("V,N", sorted(sc.CE_NEGINF))
def test_ce_neginf_oracle(V, N):
    masked = sc.CE_NEGINF[(V, N)]
    x, target, g_rows = sc.ce_case(V, N, masked)
    assert x[:, masked].isneginf().all() and not torch.isin(target, torch.tensor(masked)).any()
    assert x.isfinite().sum(1).min() >= V - len(masked)
    got = _ce_fallback(x, target, g_rows)
    for reduction in ("mean", "none"):
        ref_loss, ref_grad = oracle(x.float(), target, reduction, g_rows)
        loss, grad = got[reduction]
        assert ref_loss.isfinite().all() and ref_grad.isfinite().all()
        assert torch.allclose(loss.float(), ref_loss, **LOSS_TOL)
        assert torch.allclose(grad.float(), ref_grad, **GRAD_TOL)
        assert not grad[:, masked].any()


# ---------------------------------------------------------------------------
# AdamW, scale_
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("beta2", [0.95, 0.999])
@pytest.mark.parametrize("with_master", [True, False])
@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", sc.FLAT_SIZES[:3])
def test_adamw_oracle(n, grad_dtype, with_master, beta2):
    sc.adamw_run_and_check(n, grad_dtype, with_master, beta2, "cpu")


def test_adamw_oracle_past_the_grid_cap():
    sc.adamw_run_and_check(sc.FLAT_SIZES[3], torch.float32, False, 0.95, "cpu")


def test_adamw_nonfinite_grad_oracle():
    sc.adamw_nonfinite_check("cpu")


@pytest.mark.parametrize("as_tensor", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", sc.FLAT_SIZES)
def test_scale_oracle(n, dtype, as_tensor):
    sc.scale_run_and_check(n, dtype, as_tensor, "cpu")


def test_arena_notices_a_stray_write():
    arena = sc.Arena([torch.zeros(5), torch.zeros(8)], "cpu")
    assert arena.intact() and arena.views[1].data_ptr() % 32 == 0
    arena.views[0].fill_(1.0)
    assert arena.intact()
    arena.arena[sc.PAD + 5] = 0.0  # the element after the first slice
    assert not arena.intact()


# ---------------------------------------------------------------------------
# RoPE, RMSNorm
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pos_offset", sc.ROPE_OFFSETS)
@pytest.mark.parametrize("B,S,H,D", sc.ROPE_SHAPES)
def test_rope_oracle(B, S, H, D, pos_offset):
    from vescale_amd.ops.functional import _rope_ref

    x, table = sc.rope_case(B, S, H, D)
    assert table.shape[0] > S + pos_offset
    for backward in (False, True):
        ref, mag = sc.rope_oracle(x, table, pos_offset, backward)
        got = _rope_ref(x, table, pos_offset, backward)
        assert got.dtype == torch.bfloat16
        assert bool(((got.double() - ref).abs() <= sc.rope_bound(ref, mag)).all())
    # a rotation: norms of the pairs are kept, backward undoes forward
    ref, _ = sc.rope_oracle(x, table, pos_offset, False)
    rot = D // 2
    n2 = ref[..., :rot] ** 2 + ref[..., rot:] ** 2
    x2 = x.double()[..., :rot] ** 2 + x.double()[..., rot:] ** 2
    assert torch.allclose(n2, x2, rtol=1e-6, atol=0)


@pytest.mark.parametrize("hidden", sc.RMS_HIDDEN)
@pytest.mark.parametrize("rows", sc.RMS_ROWS)
def test_rmsnorm_oracle(rows, hidden):
    from vescale_amd.ops import fused_add_rmsnorm, rmsnorm

    x, res, w = sc.rms_case(rows, hidden)
    ref_out, ref_res, ref_rrms = sc.rms_oracle(x, None, w)
    assert torch.allclose(rmsnorm(x, w, sc.RMS_EPS).double(), ref_out, **sc.RMS_OUT_TOL)
    # the fallback's own fp32 rrms
    rrms32 = torch.rsqrt(x.float().pow(2).mean(-1) + sc.RMS_EPS)
    assert bool(((rrms32.double() - ref_rrms).abs() <= sc.rms_rrms_rtol(hidden) * ref_rrms).all())
    for r in (None, res):
        ref_out, ref_res, _ = sc.rms_oracle(x, r, w)
        out, res_new = fused_add_rmsnorm(x, r, w, sc.RMS_EPS)
        assert sc.same_bits(res_new, ref_res)
        assert torch.allclose(out.double(), ref_out, **sc.RMS_OUT_TOL)
