"""Cases and oracles for the dense MFMA GEMMs: gemm_tn (csrc/gemm.hip, five
tile geometries) and gemm_tn8 (csrc/gemm8.hip, nine schedules), both
C[M,N] = A[M,K] @ B[N,K]^T with bf16 operands, fp32 accumulation and a bf16
result rounded to nearest even.

Two tiers use this module.  test_gemm_dense.py (CPU) proves that the inputs
keep the oracles exact and that a correct GEMM meets the rounding bound;
test_gemm_dense_gpu.py holds the HIP kernels to the same oracles at the same
cases.  Every generator is a function of its parameters alone: seeded, built
on the CPU, cached so that a reference is computed once.
"""
import functools

import torch

# gemm_tn variant -> (BM, BN, BK, NBUF): the tile and pipeline depth that
# extension.hip and gemm.hip give it
TN_VARIANTS = {0: (256, 256, 32, 4), 1: (128, 256, 64, 3), 2: (256, 256, 32, 4),
               3: (128, 128, 32, 4), 4: (512, 256, 32, 3)}
G8_BM, G8_BN, G8_BK = 256, 256, 64
G8_MODES = tuple(range(9))
DEEP_K = 4160  # 130 / 65 K-tiles; the largest K of any exact case
# grids in tiles (M tiles, N tiles): nwg = 9 (q = 1, r = 1), 10 (r = 2) and 15
# (r = 7) for the XCD remap; the last two are not square, which a swap of the
# two tile coordinates cannot survive
GRIDS = ((3, 3), (2, 5), (5, 3))


def tn_ktiles(variant):
    """K-tile counts around the pipeline depth NBUF: the prologue stages
    min(NBUF-1, KT) tiles, and the counted wait changes as KT - kt drops
    below it."""
    nbuf = TN_VARIANTS[variant][3]
    return sorted({1, 2, nbuf - 1, nbuf, nbuf + 1, 2 * nbuf + 1})


def g8_ktile_ok(mode, ntile):
    """The host guards of gemm_tn8."""
    if mode == 5:
        return ntile % 2 == 0
    if mode in (7, 8):
        return ntile % 2 == 0 and ntile >= 4
    return True


def g8_ktiles(mode):
    return [n for n in range(1, 9) if g8_ktile_ok(mode, n)]


def g8_deep_k(mode):
    return DEEP_K if g8_ktile_ok(mode, DEEP_K // G8_BK) else 4096


def g8_filled_k(mode):
    """The filled-machine probe: 3 K-tiles where the mode takes them, else 4."""
    return 192 if g8_ktile_ok(mode, 3) else 256


def grid_ks(bm, bk, ok=lambda ntile: True):
    """(K of the exact grid case, K of the placement grid case): the smallest
    allowed K of at least two tiles, and the smallest allowed K that does not
    divide BM, so that i % K differs between tile rows."""
    counts = [n for n in range(2, 9) if ok(n)]
    return counts[0] * bk, next(n * bk for n in counts if bm % (n * bk))


# ---------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(M, N, K):
    """(a [M,K], b [N,K]) bf16 holding integers drawn uniformly from -4..4.
    Every product (|.| <= 16), every partial sum in any order and the full sum
    (|.| <= 16 K < 2^24) are integers that fp32 holds exactly, so a kernel
    that accumulates in fp32 must give the rounding of the true product
    whatever its summation order."""
    assert 16 * K < 2 ** 24
    gen = torch.Generator().manual_seed(1_000_003 * M + 1009 * N + K)
    a = torch.randint(-4, 5, (M, K), generator=gen).bfloat16()
    b = torch.randint(-4, 5, (N, K), generator=gen).bfloat16()
    return a, b


@functools.lru_cache(maxsize=None)
def placement_case(M, N, K):
    """Row i of a is one-hot at k = i % K; b[j, k] = (j % 7) - 3 + (k % 5) is
    not symmetric.  So c[i, j] = b[j, i % K] names its row and its column."""
    a = torch.zeros(M, K)
    a[torch.arange(M), torch.arange(M) % K] = 1.0
    j, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    b = ((j % 7) - 3 + (k % 5)).float()
    return a.bfloat16(), b.bfloat16()


def product64(a, b):
    return a.double() @ b.double().t()


_expected = {}


def exact_expected(a, b):
    """The one bf16 result an exact case allows: the fp64 product is exact,
    its fp32 value is the same integer, and the kernel's f32_to_bf16 rounds to
    nearest even like torch.  Cached per operand pair."""
    key = (a.data_ptr(), b.data_ptr())
    if key not in _expected:
        _expected[key] = (a, b, product64(a, b).float().bfloat16())
    return _expected[key][2]


def assert_exact(got, a, b, tag, bm=None, bn=None):
    """got equals exact_expected as values (torch.equal: a NaN fails; the sign
    of a zero is not compared, the oracle's own sum order could set it)."""
    want = exact_expected(a, b)
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    if torch.equal(got, want):
        return
    bad = (got != want) | got.isnan()
    i, j = (int(v) for v in bad.nonzero()[0])
    where = f", tile ({i // bm}, {j // bn})" if bm else ""
    rows, cols = bad.any(1).sum().item(), bad.any(0).sum().item()
    raise AssertionError(
        f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ, in {rows} rows and {cols} "
        f"columns; first at [{i}, {j}]{where}: got {got[i, j].item()}, want {want[i, j].item()}")


# ---------------------------------------------------------------------------
# rounding case
# ---------------------------------------------------------------------------
ROUNDING_SHAPE = (512, 768, 1088)  # 2 x 3 tiles of 256; 34 / 17 K-tiles


@functools.lru_cache(maxsize=None)
def rounding_case(M, N, K):
    """(a, b) bf16, randn / 8."""
    gen = torch.Generator().manual_seed(77_003 * M + 313 * N + K)
    a = (torch.randn(M, K, generator=gen) / 8).bfloat16()
    b = (torch.randn(N, K, generator=gen) / 8).bfloat16()
    return a, b


def rounding_bound(a, b):
    """(ref, bound), fp64, for got = bf16(fp32-accumulated a @ b^T):
        |got - ref| <= 2^-8 |ref| + K 2^-23 (|a| @ |b|^T).
    First term: one round to nearest of the result to bf16 (8 significant
    bits) moves it by at most 2^-9 of its magnitude; twice that is allowed.
    Second term: the products of bf16 numbers are exact in fp32, and a sum of K
    terms in any order picks up at most (K - 1) roundings of 2^-24 relative to
    a partial sum no larger than sum |a_k b_k|; K 2^-23 is twice that."""
    K = a.shape[1]
    ref = product64(a, b)
    return ref, 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * product64(a.abs(), b.abs())


def assert_within_rounding(got, a, b, tag):
    ref, bound = rounding_bound(a, b)
    err = (got.cpu().double() - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{tag}: max |err| / bound = {worst:.3f}, max |err| = {err.max().item():.3e}")
    assert bool((err <= bound).all()), (tag, worst)


# ---------------------------------------------------------------------------
# every exact (M, N, K) the GPU tier launches, for the CPU tier's self-check
# ---------------------------------------------------------------------------
FILLED_MN = 4096
G8_FILLED_MODES = tuple(range(2, 9))


def tn_exact_shapes(variant):
    bm, bn, bk, _ = TN_VARIANTS[variant]
    shapes = [(bm, bn, n * bk) for n in tn_ktiles(variant)] + [(bm, bn, DEEP_K)]
    shapes += [(gm * bm, gn * bn, grid_ks(bm, bk)[0]) for gm, gn in GRIDS]
    return shapes


def g8_exact_shapes(mode):
    ok = functools.partial(g8_ktile_ok, mode)
    shapes = [(G8_BM, G8_BN, n * G8_BK) for n in g8_ktiles(mode)]
    shapes.append((G8_BM, G8_BN, g8_deep_k(mode)))
    shapes += [(gm * G8_BM, gn * G8_BN, grid_ks(G8_BM, G8_BK, ok)[0]) for gm, gn in GRIDS]
    if mode in G8_FILLED_MODES:
        shapes.append((FILLED_MN, FILLED_MN, g8_filled_k(mode)))
    return shapes


def all_exact_shapes():
    shapes = set()
    for v in TN_VARIANTS:
        shapes.update(tn_exact_shapes(v))
    for m in G8_MODES:
        shapes.update(g8_exact_shapes(m))
    return sorted(shapes)


def placement_shapes():
    shapes = set()
    for bm, bn, bk, _ in TN_VARIANTS.values():
        shapes.update((gm * bm, gn * bn, grid_ks(bm, bk)[1]) for gm, gn in GRIDS)
    for m in G8_MODES:
        k = grid_ks(G8_BM, G8_BK, functools.partial(g8_ktile_ok, m))[1]
        shapes.update((gm * G8_BM, gn * G8_BN, k) for gm, gn in GRIDS)
    return sorted(shapes)


# ---------------------------------------------------------------------------
# _Linear8 / linear() under VESCALE_GEMM=gemm8
# ---------------------------------------------------------------------------
# name -> (x shape, w shape, how x is made)
LINEAR8_CASES = {
    # forward in-tree with 3 K-tiles; dgrad on the library (192 % 256 != 0)
    "fwd_in_tree_3_ktiles": ((2, 128, 192), (512, 192), "plain"),
    # forward and dgrad both in-tree
    "both_in_tree": ((256, 256), (256, 256), "plain"),
    # x is every second column of a [256, 512] buffer
    "noncontiguous_x": ((256, 256), (256, 256), "strided"),
    # M = 250: both fall back to the library
    "both_fall_back": ((250, 256), (256, 256), "plain"),
}


@functools.lru_cache(maxsize=None)
def linear8_case(name):
    """(x, w, dy) bf16 on the CPU, randn / 8; x contiguous here, the GPU test
    makes the strided view."""
    xs, ws, _ = LINEAR8_CASES[name]
    gen = torch.Generator().manual_seed(4242 + sum(map(ord, name)))
    x = (torch.randn(*xs, generator=gen) / 8).bfloat16()
    w = (torch.randn(*ws, generator=gen) / 8).bfloat16()
    dy = (torch.randn(*xs[:-1], ws[0], generator=gen) / 8).bfloat16()
    return x, w, dy


def linear8_oracle(x, w, dy):
    """fp64 autograd of y = x @ w^T: (y, dx, dw), and for each the rounding
    bound of the GEMM that produces it (contraction over K, N and M)."""
    x64 = x.double().requires_grad_()
    w64 = w.double().requires_grad_()
    y = torch.nn.functional.linear(x64, w64)
    y.backward(dy.double())
    x2, dy2 = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
    bounds = (rounding_bound(x2, w)[1].reshape(y.shape),
              rounding_bound(dy2, w.t())[1].reshape(x.shape),
              rounding_bound(dy2.t(), x2.t())[1])
    return (y.detach(), x64.grad, w64.grad), bounds
