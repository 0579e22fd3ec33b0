"""Cases, fp64 oracles and a numpy Philox4x32-10 for the streaming
(memory-bound) kernels: swiglu, dense cross-entropy, AdamW, scale_, rope,
rmsnorm forward and the philox fills.

Two tiers use this module.  test_streaming_edges.py (CPU) holds the oracles
against the torch fallbacks of ops/functional.py and the Philox reference
against the Random123 known answers; test_streaming_edges_gpu.py and
test_philox_reference_gpu.py hold the HIP kernels against the same oracles at
the same cases.  Every generator is a function of its parameters alone:
seeded, built on the CPU.
"""
import math

import numpy as np
import torch

from tests.vp_ce_cases import IGNORE, boundary_targets

PAD = 4096  # NaN elements on each side of every arena slice
# flat sizes: tail only in one block; one vector and no tail; many vectors and
# a tail; past the 2048-block x 256-thread x 8-element grid cap, with a tail
FLAT_SIZES = [5, 8, 2051, 2048 * 256 * 8 + 13]


# ---------------------------------------------------------------------------
# guard arenas
# ---------------------------------------------------------------------------
def nan_bits(dtype):
    it = torch.int16 if dtype == torch.bfloat16 else torch.int32
    return it, torch.tensor(float("nan"), dtype=dtype).view(it).item()


class Arena:
    """Same-dtype tensors as contiguous slices of one all-NaN 1-D arena on
    `device`, PAD elements before, between and after them; every slice starts
    at a multiple of 8 elements.  intact() is true while every element outside
    the slices still has the NaN's bit pattern."""

    def __init__(self, tensors, device):
        dtype = tensors[0].dtype
        assert all(t.dtype == dtype for t in tensors)
        spans, off = [], PAD
        for t in tensors:
            spans.append((off, t.numel()))
            off += (t.numel() + 7) // 8 * 8 + PAD
        self.arena = torch.full((off,), float("nan"), dtype=dtype, device=device)
        self.outside = torch.ones(off, dtype=torch.bool, device=device)
        self.views = []
        for t, (a, n) in zip(tensors, spans):
            self.arena[a:a + n] = t.reshape(-1).to(device)
            self.outside[a:a + n] = False
            self.views.append(self.arena[a:a + n].view(t.shape))
        assert all(v.data_ptr() % 16 == 0 for v in self.views)

    def intact(self):
        it, bits = nan_bits(self.arena.dtype)
        if self.arena.is_cuda:
            torch.cuda.synchronize()
        return bool((self.arena.view(it)[self.outside] == bits).all())


def same_bits(a, b):
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------
SWIGLU_PACKED_SHAPES = [(1, 16), (3, 48), (37, 2064), (4099, 2064)]
SWIGLU_OUT_TOL = dict(atol=2e-2, rtol=2e-2)   # test_swiglu / test_swiglu_packed
SWIGLU_GRAD_TOL = dict(atol=3e-2, rtol=3e-2)


def swiglu_case(n, seed=0):
    """(gate, up, dy) bf16 [n]."""
    gen = torch.Generator().manual_seed(7000 + 31 * seed + n % 100003)
    g = torch.randn(n, generator=gen) * 3
    u = torch.randn(n, generator=gen) * 2
    dy = torch.randn(n, generator=gen)
    return g.bfloat16(), u.bfloat16(), dy.bfloat16()


def swiglu_packed_case(rows, F2):
    """(gu [rows, F2], dy [rows, F2/2]) bf16."""
    g, u, dy = swiglu_case(rows * (F2 // 2), seed=F2)
    F = F2 // 2
    gu = torch.cat([g.view(rows, F), u.view(rows, F)], dim=-1).contiguous()
    return gu, dy.view(rows, F).contiguous()


def swiglu_special_case():
    """Every gate in +-{0, 30, 88, 100, 3e38} with every (up, dy) of a set
    that reaches 1e18: exp(-gate) overflows or underflows fp32, and silu, up
    and dy overflow bf16 in the output while up * dy (1e36) is still an fp32
    number.  150 elements: 18 vectors and a tail of 6."""
    gates = [s * v for v in (0.0, 30.0, 88.0, 100.0, 3e38) for s in (1.0, -1.0)]
    ups = [1.0, -2.5, 1e18, -1e18, 1e-30]
    dys = [1.0, -1e18, 1e18]
    grid = torch.tensor([(g, u, d) for g in gates for u in ups for d in dys])
    g, u, dy = (grid[:, i].bfloat16().contiguous() for i in range(3))
    return g, u, dy


def swiglu_oracle(g, u, dy):
    """fp64 (out, dgate, dup): silu(g) * u and its analytic gradients."""
    g, u, dy = g.double(), u.double(), dy.double()
    sig = 1.0 / (1.0 + torch.exp(-g))
    silu = g * sig
    return silu * u, dy * u * (sig * (1.0 + g * (1.0 - sig))), dy * silu


def same_nonfinite(got, ref64):
    """got (bf16) is finite wherever ref64 rounded to bf16 is, NaN where it is
    NaN and the same infinity where it is infinite."""
    ref = ref64.bfloat16()
    return (torch.equal(got.isnan(), ref.isnan())
            and torch.equal(got.isposinf(), ref.isposinf())
            and torch.equal(got.isneginf(), ref.isneginf()))


# ---------------------------------------------------------------------------
# dense cross-entropy
# ---------------------------------------------------------------------------
# (V, N): one vector and 255 idle threads; 8 busy threads; exactly one block
# iteration; one vector past it; one vector past two; rows above the grid cap
CE_SHAPES = [(8, 37), (64, 37), (2048, 37), (2056, 37), (4104, 37), (64, 2051)]
# masked (-inf) columns: the whole first vectors of threads 0 and 1; thread
# 1's first vector and the vector past the first block iteration
CE_NEGINF = {(64, 37): list(range(0, 16)),
             (2056, 37): list(range(8, 16)) + list(range(2048, 2056))}


def ce_case(V, N, masked=()):
    """(logits [N, V] bf16, target [N], dloss_rows [N] f32).  Rows 3 and 4
    carry an offset of +1e4 / -1e4, where bf16 numbers are 64 apart; targets
    are boundary_targets' (ignore_index, first and last column, both sides of
    column 2048) plus a second ignored row.  `masked` columns are -inf in
    every row and are no row's target."""
    gen = torch.Generator().manual_seed(900001 + 1000 * V + N)
    x = torch.randn(N, V, generator=gen) * 2
    x[3] += 1e4
    x[4] -= 1e4
    bounds = [0, 2048, V] if V > 2048 else [0, V]
    target = boundary_targets(bounds, V, N, gen, extra=(IGNORE,))
    g_rows = torch.rand(N, generator=gen) + 0.5
    if len(masked):
        cols = torch.tensor(masked)
        x[:, cols] = float("-inf")
        free = next(c for c in range(V) if c not in set(masked))
        hit = (target.unsqueeze(1) == cols.unsqueeze(0)).any(1)
        target = torch.where(hit, torch.full_like(target, free), target)
    return x.bfloat16(), target, g_rows


# ---------------------------------------------------------------------------
# AdamW, scale_
# ---------------------------------------------------------------------------
ADAMW_HYPER = dict(lr=1e-3, beta1=0.9, eps=1e-8, weight_decay=0.1, grad_scale=0.25)
ADAMW_CLIP = 0.5
ADAMW_STEPS = (1, 2, 3)
# test_adamw_flat's tolerances (allclose's default rtol where it gives none)
ADAMW_MASTER_TOL = dict(atol=1e-5, rtol=1e-4)
ADAMW_M_TOL = dict(atol=1e-6, rtol=1e-5)
ADAMW_V_TOL = dict(atol=1e-7, rtol=1e-5)


def adamw_case(n, grad_dtype):
    """(param bf16, master f32, grads: one per step in grad_dtype).  The
    master is not bf16-representable, param is its rounding."""
    gen = torch.Generator().manual_seed(5000 + n % 100003)
    master = torch.randn(n, generator=gen)
    grads = [(torch.randn(n, generator=gen) * 4).to(grad_dtype) for _ in ADAMW_STEPS]
    return master.bfloat16(), master, grads


def adamw_oracle(p, g, m, v, *, beta2, step, lr, beta1, eps, weight_decay, grad_scale):
    """One fp64 AdamW step (decoupled decay, bias-corrected) from fp64 state;
    returns new (p, m, v).  grad_scale includes the clip factor."""
    g = g.double() * grad_scale
    p = p * (1 - lr * weight_decay)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    p = p - (lr / bc1) * m / ((v / bc2).sqrt() + eps)
    return p, m, v


def adamw_fp32_slack(p_old, g, m_old, v_new, *, beta2, step, lr, beta1, eps, grad_scale, **_):
    """2^-20 A: what fp32 arithmetic may add to the error of one step.  A =
    |p| + lr/bc1 (beta1 |m| + (1 - beta1) |g|) / (sqrt(v'/bc2) + eps) bounds
    the magnitude of every term the new parameter is summed from; the step
    rounds at most 16 times on the way (1 - lr wd and its product with p;
    1 - beta1, two products and a sum for m'; the same for v', halved by the
    square root; 1/bc2 and its product, the root, the sum with eps; bc1, lr/bc1
    and its product with m'; the division; the final difference), each time
    by at most 2^-24 of a value no larger than A."""
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    g = g.double().abs() * grad_scale
    upd = (lr / bc1) * (beta1 * m_old.abs() + (1 - beta1) * g) / ((v_new / bc2).sqrt() + eps)
    return 2.0 ** -20 * (p_old.abs() + upd)


NAN_ONES = 0x7FFFFFFF  # the fp32 NaN whose mantissa is all ones


def adamw_nonfinite_grads(n=29):
    """(grad f32 [n], bad positions, clean grad): inf, the default NaN and
    the all-ones NaN in the vector body (n = 3 vectors + a tail of 5) and in
    the tail; clean has 0 at the bad positions."""
    gen = torch.Generator().manual_seed(77)
    clean = torch.randn(n, generator=gen)
    bad = {1: "inf", 3: "ones", 9: "nan", 20: "ones", 25: "inf", 26: "ones", 27: "nan"}
    grad = clean.clone()
    bits = grad.view(torch.int32)
    default_nan = torch.tensor(float("nan")).view(torch.int32).item()
    for i, kind in bad.items():
        clean[i] = 0.0
        bits[i] = {"inf": 0x7F800000, "nan": default_nan, "ones": NAN_ONES}[kind]
    return grad, sorted(bad), clean


SCALE = 0.3  # not a power of two: every product is rounded


def scale_case(n, dtype):
    gen = torch.Generator().manual_seed(6000 + n % 100003)
    return (torch.randn(n, generator=gen) * 3).to(dtype)


def scale_expected(x, s=SCALE):
    """The exact result: one fp32 product by float32(s), then x's rounding."""
    s32 = torch.tensor(s, dtype=torch.float32)
    return (x.float() * s32).to(x.dtype)


# the run-and-check bodies that the CPU tier (torch fallbacks) and the GPU tier
# (HIP kernels) share: adamw_step_flat and scale_flat_ dispatch on the device
def adamw_run_and_check(n, grad_dtype, with_master, beta2, device):
    """Three steps of adamw_step_flat on arena slices against the fp64
    oracle; shared with the GPU tier."""
    from vescale_amd.ops import adamw_step_flat

    p_cpu, master_cpu, grads = adamw_case(n, grad_dtype)
    pa = Arena([p_cpu], device)
    fa = Arena([master_cpu, torch.zeros(n), torch.zeros(n)], device)
    (p,), (master, m, v) = pa.views, fa.views
    clip = torch.tensor([ADAMW_CLIP], device=device)
    hyper = dict(ADAMW_HYPER)
    gs = hyper.pop("grad_scale")
    rp = (master if with_master else p).double()
    rm, rv = torch.zeros_like(rp), torch.zeros_like(rp)
    for step, g_cpu in zip(ADAMW_STEPS, grads):
        g = g_cpu.to(device)
        if not with_master:
            rp = p.double()  # the bf16 param is the state
        adamw_step_flat(p, master if with_master else None, g, m, v, beta2=beta2,
                        step=step, grad_scale=gs, clip_scale=clip, **hyper)
        p_old, m_old = rp, rm
        rp, rm, rv = adamw_oracle(rp, g, rm, rv, beta2=beta2, step=step,
                                  grad_scale=gs * ADAMW_CLIP, **hyper)
        tag = (n, grad_dtype, with_master, beta2, step)
        assert torch.allclose(m.double(), rm, **ADAMW_M_TOL), tag
        assert torch.allclose(v.double(), rv, **ADAMW_V_TOL), tag
        if with_master:
            assert torch.allclose(master.double(), rp, **ADAMW_MASTER_TOL), tag
            assert torch.equal(p, master.bfloat16()), tag
        else:
            err = (p.double() - rp).abs()
            slack = adamw_fp32_slack(p_old, g, m_old, rv, beta2=beta2, step=step,
                                     grad_scale=gs * ADAMW_CLIP, **hyper)
            print(f"adamw no-master {tag}: max(err - 2^-7 |ref|) = "
                  f"{(err - 2.0 ** -7 * rp.abs()).max().item():.3e}, with the fp32 term "
                  f"{(err - 2.0 ** -7 * rp.abs() - slack).max().item():.3e}")
            assert bool((err <= 2.0 ** -7 * rp.abs() + slack).all()), tag
    if not with_master:
        assert same_bits(master.cpu(), master_cpu)
    assert pa.intact() and fa.intact(), (n, grad_dtype, with_master, beta2)


def adamw_nonfinite_check(device):
    """fp32 grads holding inf, the default NaN and the all-ones NaN: master
    and the bf16 param are NaN there, every other element is what the same
    step gives with zeros in their place; shared with the GPU tier."""
    from vescale_amd.ops import adamw_step_flat

    grad, bad, clean = adamw_nonfinite_grads()
    n = grad.numel()
    assert grad.view(torch.int32)[3].item() == NAN_ONES
    gen = torch.Generator().manual_seed(78)
    master0 = torch.randn(n, generator=gen)
    hyper = dict(ADAMW_HYPER, beta2=0.95, step=1)
    out = []
    for g in (grad, clean):
        p, master = master0.bfloat16().to(device), master0.clone().to(device)
        m, v = torch.zeros(n, device=device), torch.zeros(n, device=device)
        g_dev = g.to(device)
        assert same_bits(g_dev.cpu(), g)  # the payload survived the copy
        adamw_step_flat(p, master, g_dev, m, v, **hyper)
        out.append((p.cpu(), master.cpu()))
    (p, master), (p_ok, master_ok) = out
    good = torch.ones(n, dtype=torch.bool)
    good[bad] = False
    print("adamw non-finite grads: master bits",
          [hex(b & 0xFFFFFFFF) for b in master.view(torch.int32)[bad].tolist()],
          "param bits", [hex(b & 0xFFFF) for b in p.view(torch.int16)[bad].tolist()])
    assert master[bad].isnan().all()
    assert p[bad].isnan().all()
    assert same_bits(master[good], master_ok[good]) and same_bits(p[good], p_ok[good])
    assert master[good].isfinite().all()


def scale_run_and_check(n, dtype, as_tensor, device):
    from vescale_amd.ops import scale_flat_

    x_cpu = scale_case(n, dtype)
    arena = Arena([x_cpu], device)
    (x,) = arena.views
    s = torch.tensor(SCALE, device=device) if as_tensor else SCALE
    scale_flat_(x, s)
    assert same_bits(x.cpu(), scale_expected(x_cpu))
    assert arena.intact()


# ---------------------------------------------------------------------------
# RoPE (unfused)
# ---------------------------------------------------------------------------
# (B,S,H,D): 3 pairs (odd: the second pair of the last thread is past the
# end); D = 6; two batches; 1,052,672 pairs, past the 2048 x 256 x 2 cap
ROPE_SHAPES = [(1, 3, 1, 2), (1, 5, 3, 6), (2, 7, 3, 64), (1, 257, 64, 128)]
ROPE_OFFSETS = (0, 3)


def rope_case(B, S, H, D):
    """(x bf16 [B,S,H,D], table f32 [S + 5, D/2, 2])."""
    from vescale_amd.ops import build_rope_table

    gen = torch.Generator().manual_seed(8000 + 131 * S + D)
    x = torch.randn(B, S, H, D, generator=gen).bfloat16()
    return x, build_rope_table(S + 5, D, 500000.0)


def rope_oracle(x, table, pos_offset, backward):
    """fp64 rotation by the fp32 table's values; returns (out, |x0| + |x1|
    laid out like out)."""
    B, S, H, D = x.shape
    rot = D // 2
    tb = table[pos_offset:pos_offset + S].double()
    cos, sin = tb[..., 0][None, :, None, :], tb[..., 1][None, :, None, :]
    if backward:
        sin = -sin
    x0, x1 = x.double()[..., :rot], x.double()[..., rot:]
    out = torch.cat([x0 * cos - x1 * sin, x1 * cos + x0 * sin], dim=-1)
    mag = x0.abs() + x1.abs()
    return out, torch.cat([mag, mag], dim=-1)


def bf16_half_ulp(ref):
    """Half the spacing of bf16 numbers at |ref| (fp64): the largest error of
    one round-to-nearest.  bf16 has 8 significant bits, so this is 2^(e-9) for
    2^(e-1) <= |ref| < 2^e: between 2^-9 |ref| and 2^-8 |ref|."""
    _, e = torch.frexp(ref.abs())
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 9))


def rope_bound(ref, mag):
    """|err| <= half a bf16 ulp at ref + 2^-20 (|x0| + |x1|): one bf16
    rounding of the result, and a few fp32 roundings of two products of
    magnitude <= |x0| and |x1| (two products and a sum, or one product and an
    FMA).  A first term of 2^-9 |ref| cannot be met by any bf16 result: half
    an ulp is 2^-9 |ref| only where |ref| is just below a power of two and
    2^-8 |ref| just above one, so the exact half ulp is used."""
    return bf16_half_ulp(ref) + 2.0 ** -20 * mag


# ---------------------------------------------------------------------------
# RMSNorm forward, fused add + RMSNorm forward
# ---------------------------------------------------------------------------
RMS_ROWS = (1, 3, 2051)          # 2051: above the 2048-block grid cap
RMS_HIDDEN = (8, 520, 4096, 16384)  # one vector; idle lanes; 2 and 8 iterations
RMS_EPS = 1e-5
RMS_OUT_TOL = dict(atol=2e-2, rtol=2e-2)  # test_rmsnorm_fwd_bwd


def rms_case(rows, hidden):
    """(x, res, w) bf16; row 0 is 16x larger than the rest."""
    gen = torch.Generator().manual_seed(9000 + 17 * rows + hidden)
    x = torch.randn(rows, hidden, generator=gen)
    x[0] *= 16
    res = torch.randn(rows, hidden, generator=gen) * 2
    w = torch.randn(hidden, generator=gen)
    return x.bfloat16(), res.bfloat16(), w.bfloat16()


def rms_oracle(x, res, w, eps=RMS_EPS):
    """(out fp64, res_new bf16, rrms fp64): res_new is the bf16 rounding of
    the fp32 sum (x itself without res); rrms and out come from res_new."""
    res_new = x if res is None else (x.float() + res.float()).bfloat16()
    r = res_new.double()
    eps32 = float(np.float32(eps))
    rrms = torch.rsqrt(r.pow(2).mean(-1) + eps32)
    return r * rrms[:, None] * w.double(), res_new, rrms


def rms_rrms_rtol(hidden):
    """Relative bound on the fp32 rrms, see test_rmsnorm_rrms in
    test_streaming_edges_gpu.py."""
    return 2.0 ** -22 + (hidden / 8 / 256 + 16) * 2.0 ** -24


# ---------------------------------------------------------------------------
# Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
# as 1, 2, 3", SC'11), numpy
# ---------------------------------------------------------------------------
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints.
    Returns the four output words as uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _MASK,
                          (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _MASK)
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def kernel_words(seed, offset, g, stream):
    """[len(g), 4] uint32: the four words of the counter that the fill
    kernels give global element g: counter (lo32, hi32 of (g >> 2) + offset,
    stream, 0), key (lo32, hi32 of seed)."""
    g = np.asarray(g, dtype=np.uint64)
    ctr = (g >> np.uint64(2)) + np.uint64(offset & 0xFFFFFFFFFFFFFFFF)  # wraps mod 2^64
    zeros = np.zeros_like(ctr)
    w = philox4x32_10((ctr & _MASK, ctr >> _S32, zeros + np.uint64(stream), zeros),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return np.stack(w, axis=-1)


def word_to_uniform(w):
    """(float32(w) + 1) * 2^-32 in fp32: a uniform in (0, 1]."""
    return (w.astype(np.float32) + np.float32(1.0)) * np.float32(2.0 ** -32)


def ref_uniform(seed, offset, g):
    """fp32 uniforms of the global elements g (stream 0, component g & 3)."""
    g = np.asarray(g, dtype=np.uint64)
    w = kernel_words(seed, offset, g, 0)
    return word_to_uniform(w[np.arange(len(g)), (g & np.uint64(3)).astype(np.int64)])


def ref_normal64(seed, offset, g):
    """fp64 Box-Muller of the four fp32 uniforms of each counter (stream 1):
    components 0, 1 = r cos, r sin of words (0, 1); 2, 3 of words (2, 3)."""
    g = np.asarray(g, dtype=np.uint64)
    u = word_to_uniform(kernel_words(seed, offset, g, 1)).astype(np.float64)
    r01, r23 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a01, a23 = 2.0 * math.pi * u[:, 1], 2.0 * math.pi * u[:, 3]
    z = np.stack([r01 * np.cos(a01), r01 * np.sin(a01),
                  r23 * np.cos(a23), r23 * np.sin(a23)], axis=-1)
    return z[np.arange(len(g)), (g & np.uint64(3)).astype(np.int64)]


def shard_global_index(gshape, lshape, offset):
    """Row-major global element index of every element of the local block
    lshape at `offset` inside gshape, in the block's own row-major order."""
    idx = np.zeros(lshape, dtype=np.int64)
    stride = 1
    for d in reversed(range(len(gshape))):
        shape = [1] * len(gshape)
        shape[d] = lshape[d]
        idx = idx + ((np.arange(lshape[d]) + offset[d]) * stride).reshape(shape)
        stride *= gshape[d]
    return idx.reshape(-1)


# ---------------------------------------------------------------------------
# stream independence of two consecutive random ops
# ---------------------------------------------------------------------------
LAGS = range(-64, 65)


def _lagged(a, b, lag):
    """(a[g + lag], b[g]) over every g for which both exist."""
    n = len(a)
    if lag >= 0:
        return a[lag:], b[:n - lag]
    return a[:n + lag], b[-lag:]


def mask_agreement_violations(mask1, mask2, p_agree=0.5):
    """Lags L in -64..64 at which the fraction of positions with mask2[g] ==
    mask1[g + L] leaves p_agree +- 5 sqrt(p_agree (1 - p_agree) / (n - |L|)):
    five standard deviations of that fraction for independent masks."""
    m1, m2 = np.asarray(mask1).reshape(-1), np.asarray(mask2).reshape(-1)
    bad = []
    for lag in LAGS:
        a, b = _lagged(m1, m2, lag)
        frac = float((a == b).mean())
        if abs(frac - p_agree) > 5 * math.sqrt(p_agree * (1 - p_agree) / len(a)):
            bad.append((lag, frac))
    return bad


def max_equal_values(x1, x2):
    """Largest number, over the lags -64..64, of positions at which x2[g] and
    x1[g + L] have the same bits; with the lag it was found at."""
    a1 = np.asarray(x1).reshape(-1).view(np.uint32)
    a2 = np.asarray(x2).reshape(-1).view(np.uint32)
    best = (0, 0)
    for lag in LAGS:
        a, b = _lagged(a1, a2, lag)
        best = max(best, (int((a == b).sum()), lag))
    return best
