"""The streaming (memory-bound) HIP kernels at the shapes where their loop
structure changes - scalar tails, fewer elements than one vector, idle
threads, row div/mod with a non-power-of-two divisor, grid-stride loops past
the block cap - against the fp64 oracles of tests/streaming_cases.py, which
test_streaming_edges.py verifies on the CPU.  Every buffer a kernel writes in
place is a slice of a NaN-filled arena that must come back untouched.

Where a tolerance is not derived in a docstring here, it is the named
existing test's: test_swiglu / test_swiglu_packed, test_fused_cross_entropy
(LOSS_TOL, GRAD_TOL of vp_ce_cases.py), test_adamw_flat, test_rmsnorm_fwd_bwd.
"""
import functools

import pytest
import torch

from tests import streaming_cases as sc
from tests.vp_ce_cases import GRAD_TOL, IGNORE, LOSS_TOL, oracle

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")


def _ext():
    import vescale_amd.ops as ops

    return ops.require_ext()


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------
def _swiglu_gpu(g, u, dy):
    C = _ext()
    g, u, dy = g.cuda(), u.cuda(), dy.cuda()
    out = C.swiglu_fwd(g, u)
    dg, du = C.swiglu_bwd(dy, g, u)
    return out, dg, du


@requires_gpu
@pytest.mark.parametrize("n", sc.FLAT_SIZES)
def test_swiglu_flat_sizes(n):
    g, u, dy = sc.swiglu_case(n)
    out, dg, du = _swiglu_gpu(g, u, dy)
    r_out, r_dg, r_du = (r.cuda() for r in sc.swiglu_oracle(g, u, dy))
    assert out.shape == (n,) and dg.shape == (n,) and du.shape == (n,)
    assert torch.allclose(out.double(), r_out, **sc.SWIGLU_OUT_TOL)
    assert torch.allclose(dg.double(), r_dg, **sc.SWIGLU_GRAD_TOL)
    assert torch.allclose(du.double(), r_du, **sc.SWIGLU_GRAD_TOL)
    again = _swiglu_gpu(g, u, dy)
    assert all(sc.same_bits(a, b) for a, b in zip((out, dg, du), again))


@requires_gpu
@pytest.mark.parametrize("rows,F2", sc.SWIGLU_PACKED_SHAPES)
def test_swiglu_packed_shapes(rows, F2):
    """F/8 = 129 vectors per row is no power of two, and 4099 * 129 vectors
    are more than 2048 * 256 threads.  The packed and the separate kernels do
    the same arithmetic: their results are bitwise equal."""
    C = _ext()
    gu_cpu, dy_cpu = sc.swiglu_packed_case(rows, F2)
    F = F2 // 2
    gu, dy = gu_cpu.cuda(), dy_cpu.cuda()
    out = C.swiglu_packed_fwd(gu)
    dgu = C.swiglu_packed_bwd(dy, gu)
    r_out, r_dg, r_du = (r.cuda() for r in sc.swiglu_oracle(gu_cpu[:, :F], gu_cpu[:, F:], dy_cpu))
    assert out.shape == (rows, F) and dgu.shape == (rows, F2)
    assert torch.allclose(out.double(), r_out, **sc.SWIGLU_OUT_TOL)
    assert torch.allclose(dgu.double(), torch.cat([r_dg, r_du], -1), **sc.SWIGLU_GRAD_TOL)
    s_out, s_dg, s_du = _swiglu_gpu(gu_cpu[:, :F].contiguous(), gu_cpu[:, F:].contiguous(), dy_cpu)
    assert sc.same_bits(out, s_out)
    assert sc.same_bits(dgu, torch.cat([s_dg, s_du], -1))


@requires_gpu
def test_swiglu_special_values():
    """Gates at which exp(-gate) overflows or vanishes in fp32, with up and dy
    up to 1e18: the output is finite wherever the fp64 result rounded to bf16
    is, and NaN / +inf / -inf exactly where that is.  Separate kernels (18
    vectors and a scalar tail of 6) and packed kernels (the first 144)."""
    C = _ext()
    g, u, dy = sc.swiglu_special_case()
    refs = sc.swiglu_oracle(g, u, dy)
    for name, got, ref in zip(("out", "dgate", "dup"), _swiglu_gpu(g, u, dy), refs):
        assert sc.same_nonfinite(got.cpu(), ref), name
    k = g.numel() // 16 * 16
    gu = torch.cat([g[:k].view(-1, 16), u[:k].view(-1, 16)], -1).contiguous().cuda()
    out = C.swiglu_packed_fwd(gu)
    dgu = C.swiglu_packed_bwd(dy[:k].view(-1, 16).contiguous().cuda(), gu)
    assert sc.same_nonfinite(out.cpu().reshape(-1), refs[0][:k])
    assert sc.same_nonfinite(dgu[:, :16].cpu().reshape(-1), refs[1][:k])
    assert sc.same_nonfinite(dgu[:, 16:].cpu().reshape(-1), refs[2][:k])


# ---------------------------------------------------------------------------
# dense cross-entropy
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ce_results(V, N, masked=()):
    from vescale_amd.ops import fused_cross_entropy

    C = _ext()
    x_cpu, t_cpu, g_cpu = sc.ce_case(V, N, masked)
    arena = sc.Arena([x_cpu], "cuda")
    (x,) = arena.views
    target, g_rows = t_cpu.cuda(), g_cpu.cuda()
    rows, lse = C.ce_fwd(x, target, IGNORE)
    rows2, lse2 = C.ce_fwd(x, target, IGNORE)
    xm = x.detach().requires_grad_(True)
    mean = fused_cross_entropy(xm, target, IGNORE)
    mean.backward()
    grad_rows = C.ce_bwd(x, target, lse, g_rows, IGNORE, False)
    grad_rows2 = C.ce_bwd(x, target, lse, g_rows, IGNORE, False)
    assert grad_rows.data_ptr() != x.data_ptr()
    saved = x.clone()
    inplace = C.ce_bwd(x, target, lse, g_rows, IGNORE, True)
    assert inplace.data_ptr() == x.data_ptr()
    inplace = inplace.clone()
    x.copy_(saved)
    return dict(x=x, x_cpu=x_cpu, target=target, g_rows=g_rows, rows=rows, lse=lse,
                rows2=rows2, lse2=lse2, mean=mean.detach(), grad_mean=xm.grad,
                grad_rows=grad_rows, grad_rows2=grad_rows2, inplace=inplace,
                arena_ok=arena.intact())


@requires_gpu
@pytest.mark.parametrize("V,N", sc.CE_SHAPES)
def test_ce_dense_shapes(V, N):
    """V < 2048 leaves threads without a column; V = 2056 and 4104 give
    thread 0 one vector more than the rest; N = 2051 makes blocks loop over
    rows.  Rows 3 and 4 sit at +-1e4, where bf16 numbers are 64 apart."""
    r = _ce_results(V, N)
    x64, target, g_rows = r["x"].double(), r["target"], r["g_rows"]
    lse_ref = torch.logsumexp(x64, dim=-1)
    print(f"ce V={V} N={N}: lse err {(r['lse'].double() - lse_ref).abs().max().item():.3e}")
    assert torch.allclose(r["lse"].double(), lse_ref, **LOSS_TOL)
    ref_mean, ref_gmean = oracle(x64, target, "mean")
    ref_rows, ref_grows = oracle(x64, target, "none", g_rows)
    assert torch.allclose(r["mean"].double(), ref_mean, **LOSS_TOL)
    assert torch.allclose(r["rows"].double(), ref_rows, **LOSS_TOL)
    assert torch.allclose(r["grad_mean"].double(), ref_gmean, **GRAD_TOL)
    assert torch.allclose(r["grad_rows"].double(), ref_grows, **GRAD_TOL)
    ignored = target == IGNORE
    assert ignored.sum() == 2
    assert not r["rows"][ignored].any()
    assert not r["grad_mean"][ignored].any() and not r["grad_rows"][ignored].any()


@requires_gpu
@pytest.mark.parametrize("V,N", sc.CE_SHAPES)
def test_ce_dense_inplace_and_repeatable(V, N):
    r = _ce_results(V, N)
    assert r["arena_ok"]
    assert sc.same_bits(r["inplace"], r["grad_rows"])
    assert sc.same_bits(r["grad_rows"], r["grad_rows2"])
    assert sc.same_bits(r["rows"], r["rows2"]) and sc.same_bits(r["lse"], r["lse2"])


@requires_gpu
@pytest.mark.parametrize("V,N", sorted(sc.CE_NEGINF))
def test_ce_dense_neginf_logits(V, N):
    """Masked (-inf) columns that fill a thread's first vector: the online
    max/sum update must not form exp(-inf - -inf).  Loss and lse are finite
    and F.cross_entropy's in fp32; the gradient is +-0 at the masked columns."""
    masked = tuple(sc.CE_NEGINF[(V, N)])
    r = _ce_results(V, N, masked)
    x32, target, g_rows = r["x"].float(), r["target"], r["g_rows"]
    assert x32[:, list(masked)].isneginf().all()
    lse_ref = torch.logsumexp(x32, dim=-1)
    ref_mean, ref_gmean = oracle(x32, target, "mean")
    ref_rows, ref_grows = oracle(x32, target, "none", g_rows)
    print(f"ce -inf V={V} N={N}: lse nan rows {int(r['lse'].isnan().sum())} of {N}")
    assert r["lse"].isfinite().all() and r["rows"].isfinite().all() and r["mean"].isfinite()
    assert torch.allclose(r["lse"], lse_ref, **LOSS_TOL)
    assert torch.allclose(r["mean"], ref_mean, **LOSS_TOL)
    assert torch.allclose(r["rows"], ref_rows, **LOSS_TOL)
    for got, ref in ((r["grad_mean"], ref_gmean), (r["grad_rows"], ref_grows)):
        assert not got[:, list(masked)].any()
        assert torch.allclose(got.float(), ref, **GRAD_TOL)
    assert r["arena_ok"] and sc.same_bits(r["inplace"], r["grad_rows"])


# ---------------------------------------------------------------------------
# AdamW, scale_
# ---------------------------------------------------------------------------
@requires_gpu
@pytest.mark.parametrize("beta2", [0.95, 0.999])
@pytest.mark.parametrize("with_master", [True, False])
@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", sc.FLAT_SIZES)
def test_adamw_flat_sizes(n, grad_dtype, with_master, beta2):
    """Steps 1..3 with grad_scale 0.25 and a clip tensor of 0.5, against an
    fp64 AdamW on the same inputs.  With a master: m, v, master at
    test_adamw_flat's tolerances and param == master.bfloat16() exactly.
    Without one the bf16 param is the state: each step is within one bf16 ulp
    (2^-7 relative) of the fp64 step taken from the bf16 param, plus the fp32
    error of the step itself, 2^-20 A (streaming_cases.adamw_fp32_slack).
    The relative term alone cannot hold for any fp32 step: where the decayed
    parameter and the update cancel, the result is far smaller than the fp32
    roundings of the two (measured on an MI355X at n = 4194317 with bf16
    grads, step 3: an error 2.4e-10 above 2^-7 |ref| at such an element).
    param, master, m and v are arena slices."""
    sc.adamw_run_and_check(n, grad_dtype, with_master, beta2, "cuda")


@requires_gpu
def test_adamw_nonfinite_grad_reaches_master_and_param():
    """inf, the default NaN and the NaN with bits 0x7FFFFFFF in an fp32 grad,
    in the vector body and in the scalar tail.  Rounding 0x7FFFFFFF to bf16 by
    adding 0x7FFF + lsb carries into the sign bit and gives 0x8000 (-0.0): a
    NaN master next to a -0.0 parameter, unless f32_to_bf16 has a NaN case."""
    sc.adamw_nonfinite_check("cuda")


@requires_gpu
@pytest.mark.parametrize("as_tensor", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", sc.FLAT_SIZES)
def test_scale_flat_sizes(n, dtype, as_tensor):
    """One fp32 product and (bf16) one rounding: exact, compared bitwise."""
    sc.scale_run_and_check(n, dtype, as_tensor, "cuda")


# ---------------------------------------------------------------------------
# RoPE (unfused)
# ---------------------------------------------------------------------------
@requires_gpu
@pytest.mark.parametrize("pos_offset", sc.ROPE_OFFSETS)
@pytest.mark.parametrize("B,S,H,D", sc.ROPE_SHAPES)
def test_rope_shapes(B, S, H, D, pos_offset):
    """Per element |err| <= half a bf16 ulp at ref + 2^-20 (|x0| + |x1|)
    (streaming_cases.rope_bound), forward and backward; in place equals out of
    place bitwise inside a guard arena.  Forward then backward returns x
    within two bf16 roundings: before its own rounding the backward's value v
    is off x by at most the forward's two output errors, which the inverse
    rotation mixes with weights <= 1 (half an ulp at each output, h0 + h1),
    plus fp32 roundings of both passes (4 * 2^-20 (|x0| + |x1|)); x is itself
    a bf16 number, so rounding v to nearest lands no farther from v than x is:
    |back - x| <= 2 (h0 + h1 + 2^-18 (|x0| + |x1|))."""
    C = _ext()
    x_cpu, tab_cpu = sc.rope_case(B, S, H, D)
    x, tab = x_cpu.cuda(), tab_cpu.cuda()
    rot = D // 2
    for backward in (False, True):
        ref, mag = (t.cuda() for t in sc.rope_oracle(x_cpu, tab_cpu, pos_offset, backward))
        got = C.rope(x, tab, pos_offset, backward, False)
        assert got.data_ptr() != x.data_ptr() and sc.same_bits(x.cpu(), x_cpu)
        excess = ((got.double() - ref).abs() - sc.rope_bound(ref, mag)).max().item()
        print(f"rope {(B, S, H, D)} off={pos_offset} bwd={backward}: max(err - bound) {excess:.3e}")
        assert excess <= 0
        arena = sc.Arena([x_cpu], "cuda")
        (xi,) = arena.views
        same = C.rope(xi, tab, pos_offset, backward, True)
        assert same.data_ptr() == xi.data_ptr()
        assert sc.same_bits(xi, got) and arena.intact()
    fwd = C.rope(x, tab, pos_offset, False, False)
    back = C.rope(fwd, tab, pos_offset, True, False)
    ref, mag = (t.cuda() for t in sc.rope_oracle(x_cpu, tab_cpu, pos_offset, False))
    h = sc.bf16_half_ulp(ref)
    h_pair = h[..., :rot] + h[..., rot:]
    bound = 2 * (torch.cat([h_pair, h_pair], -1) + 2.0 ** -18 * mag)
    assert bool(((back.double() - x.double()).abs() <= bound).all())


# ---------------------------------------------------------------------------
# RMSNorm forward, fused add + RMSNorm forward
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rms_results(rows, hidden):
    C = _ext()
    x_cpu, res_cpu, w_cpu = sc.rms_case(rows, hidden)
    x, res, w = x_cpu.cuda(), res_cpu.cuda(), w_cpu.cuda()
    out = {"plain": C.rmsnorm_fwd(x, w, sc.RMS_EPS), "plain2": C.rmsnorm_fwd(x, w, sc.RMS_EPS)}
    for name, r in (("nores", None), ("res", res)):
        out[name] = C.rmsnorm_res_fwd(x, r, w, sc.RMS_EPS)
        out[name + "2"] = C.rmsnorm_res_fwd(x, r, w, sc.RMS_EPS)
    torch.cuda.synchronize()
    assert sc.same_bits(x.cpu(), x_cpu) and sc.same_bits(res.cpu(), res_cpu)
    return x, res, w, out


@requires_gpu
@pytest.mark.parametrize("hidden", sc.RMS_HIDDEN)
@pytest.mark.parametrize("rows", sc.RMS_ROWS)
def test_rmsnorm_rrms(rows, hidden):
    """rrms = rsqrt(mean(x^2) + eps) in fp32 against fp64, relative bound
    2^-22 + (hidden/8/256 + 16) 2^-24.  The squares of bf16 numbers are exact
    in fp32.  A thread adds hidden/256 of them in a chain (8 per iteration,
    hidden/8/256 iterations), a wave tree adds 6 levels, the block tree 2, then
    come the division by hidden and the sum with eps: at most (hidden/256 + 10)
    roundings of 2^-24 each on a sum of non-negative terms, so that much
    relative error.  The inverse square root halves a relative error:
    (hidden/512 + 5) 2^-24 <= (hidden/8/256 + 16) 2^-24 for every hidden up to
    16384.  rsqrtf itself is within 2 ulp, 2^-22."""
    x, res, w, out = _rms_results(rows, hidden)
    for name, r in (("plain", None), ("nores", None), ("res", res)):
        _, _, ref = sc.rms_oracle(x, r, w)
        rrms = out[name][-1]
        assert rrms.dtype == torch.float32 and rrms.shape == (rows,)
        rel = ((rrms.double() - ref).abs() / ref).max().item()
        print(f"rrms rows={rows} hidden={hidden} {name}: rel err {rel:.3e} "
              f"bound {sc.rms_rrms_rtol(hidden):.3e}")
        assert rel <= sc.rms_rrms_rtol(hidden), name


@requires_gpu
@pytest.mark.parametrize("hidden", sc.RMS_HIDDEN)
@pytest.mark.parametrize("rows", sc.RMS_ROWS)
def test_rmsnorm_out_and_res_new(rows, hidden):
    """res_new is the bf16 rounding of the fp32 sum (x itself without res),
    bitwise; out is the norm of that rounded res_new; calls repeat bitwise."""
    x, res, w, out = _rms_results(rows, hidden)
    ref_out, _, _ = sc.rms_oracle(x, None, w)
    assert torch.allclose(out["plain"][0].double(), ref_out, **sc.RMS_OUT_TOL)
    for name, r in (("nores", None), ("res", res)):
        ref_out, ref_res, _ = sc.rms_oracle(x, r, w)
        got_out, got_res, _ = out[name]
        assert sc.same_bits(got_res, ref_res), name
        assert torch.allclose(got_out.double(), ref_out, **sc.RMS_OUT_TOL), name
    assert sc.same_bits(out["nores"][0], out["plain"][0])
    assert sc.same_bits(out["nores"][2], out["plain"][1])  # rrms
    for name in ("plain", "nores", "res"):
        assert all(sc.same_bits(a, b) for a, b in zip(out[name], out[name + "2"])), name
