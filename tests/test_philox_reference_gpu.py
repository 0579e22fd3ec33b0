"""The sharded-philox fills (ops/csrc/philox_random.hip) against an independent
Philox4x32-10: the numpy reference of tests/streaming_cases.py, written from
the published algorithm and checked against the Random123 known answers in
test_streaming_edges.py.  Layout reproduced: counter (lo32, hi32 of
(g >> 2) + offset, stream, 0) with stream 0 for uniform and dropout and 1 for
normal, key (lo32, hi32 of seed), component g & 3 for global element g.

The last two tests run two consecutive random ops through the "thread" RNG
tracker: they must draw from disjoint counter ranges.
"""
import numpy as np
import pytest
import torch

from tests import streaming_cases as sc

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

SEEDS = (1234, (1 << 40) + 7)
OFFSETS = (0, (1 << 32) - 1)  # the second carries into the counter's second word
# (gshape, lshape, offset, flat_offset, is_flat): flat at 0 and at 5 (not a
# multiple of 4: the first counter is entered at component 1), a 3-D block
LAYOUTS = [
    ([4099], [4099], [0], 0, True),
    ([4200], [4099], [5], 5, True),
    ([5, 6, 7], [2, 3, 4], [1, 2, 3], 0, False),
]
# max |z - fp64 Box-Muller| of philox_normal_f32 measured on an MI355X over
# 2^20 elements at each of the two SEEDS (profiles/streaming_edges_gpu.txt);
# the test allows 4x as margin for other seeds and counters
NORMAL_MEASURED_ERR = 1.92e-6  # seed 1234: 1.615e-6, seed 2^40 + 7: 1.918e-6


def _ext():
    import vescale_amd.ops as ops

    return ops.require_ext()


def _global_index(layout):
    gshape, lshape, offs, foff, flat = layout
    if flat:
        return np.arange(lshape[0]) + foff
    return sc.shard_global_index(gshape, lshape, offs)


def _fill(fn, layout, dtype, seed, offset, a, b):
    gshape, lshape, offs, foff, flat = layout
    out = torch.full((int(np.prod(lshape)),), -7.0, device="cuda", dtype=dtype)
    fn(out, gshape, lshape, offs, foff, flat, seed, offset, a, b)
    return out.cpu()


@requires_gpu
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=["flat0", "flat5", "block3d"])
def test_uniform_matches_reference_bitwise(layout, seed, offset):
    """fp32 uniform(0, 1) is (float32(word) + 1) * 2^-32 exactly, bf16 its
    round-to-nearest-even; other (lo, hi) are lo + u (hi - lo) within one fp32
    ulp at hi - lo: half an ulp for the product (below 5.5, 2^-22) and half an
    ulp for the sum (below 4, 2^-23), or the latter alone if the compiler
    fuses the two into an FMA - less than 2^-21, the ulp of [4, 8)."""
    C = _ext()
    u = torch.from_numpy(sc.ref_uniform(seed, offset, _global_index(layout)))
    got = _fill(C.philox_uniform_, layout, torch.float32, seed, offset, 0.0, 1.0)
    assert sc.same_bits(got, u)
    got16 = _fill(C.philox_uniform_, layout, torch.bfloat16, seed, offset, 0.0, 1.0)
    assert sc.same_bits(got16, u.bfloat16())
    lo, hi = -3.0, 2.5
    got = _fill(C.philox_uniform_, layout, torch.float32, seed, offset, lo, hi)
    want = lo + u.double() * (hi - lo)
    ulp = 2.0 ** -21
    assert bool(((got.double() - want).abs() <= ulp).all())
    assert got.min() >= lo and got.max() <= hi


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_offset_unit_is_one_counter(dtype):
    """fill(offset=k)[g] == fill(offset=0)[g + 4k]: one unit of the philox
    offset is one counter, four elements - the unit in which the RNG tracker
    advances between ops."""
    C = _ext()
    n, k = 4096, 37
    for fn in (C.philox_uniform_, C.philox_normal_):
        base = _fill(fn, ([n + 4 * k], [n + 4 * k], [0], 0, True), dtype, 99, 0, 0.0, 1.0)
        moved = _fill(fn, ([n], [n], [0], 0, True), dtype, 99, k, 0.0, 1.0)
        assert sc.same_bits(moved, base[4 * k:])


@requires_gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["flat0", "flat5", "block3d"])
def test_dropout_matches_reference(layout, p):
    """keep = u > float32(p) from the reference uniforms, bitwise; dropped
    outputs are exactly 0; kept ones are x / (1 - p) within 2^-8 relative (one
    bf16 rounding, and fp32 roundings of the scale and the product)."""
    C = _ext()
    gshape, lshape, offs, foff, flat = layout
    seed, offset = SEEDS[1], 3
    n = int(np.prod(lshape))
    x = (torch.randn(n, generator=torch.Generator().manual_seed(n)) + 3.0).bfloat16()
    out, mask = C.philox_dropout(x.cuda(), gshape, lshape, offs, foff, flat, seed, offset, p, True)
    out, mask = out.cpu(), mask.cpu()
    keep = torch.from_numpy(sc.ref_uniform(seed, offset, _global_index(layout)) > np.float32(p))
    assert mask.dtype == torch.uint8 and torch.equal(mask.bool(), keep)
    assert not out[~keep].any()
    want = x.double()[keep] / (1.0 - p)
    assert bool(((out.double()[keep] - want).abs() <= 2.0 ** -8 * want.abs()).all())


@requires_gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_normal_against_fp64_box_muller(seed):
    """Every output is finite with |z| <= 6.67 (the smallest uniform is 2^-32:
    sqrt(-2 ln 2^-32) = 6.66), and within 4 x NORMAL_MEASURED_ERR of an fp64
    Box-Muller of the same four words per counter.  The device logf / sqrtf /
    __sincosf error is measured, not derived: max |z - ref| over 2^20 elements
    was 1.615e-6 at seed 1234 and 1.918e-6 at seed 2^40 + 7 on an MI355X
    (profiles/streaming_edges_gpu.txt); 4 x 1.92e-6 = 7.68e-6 is allowed."""
    C = _ext()
    n = 1 << 20
    got = _fill(C.philox_normal_, ([n], [n], [0], 0, True), torch.float32, seed, 0, 0.0, 1.0)
    ref = sc.ref_normal64(seed, 0, np.arange(n))
    assert got.isfinite().all() and got.abs().max() <= 6.67
    err = float(np.abs(got.double().numpy() - ref).max())
    print(f"philox normal seed={seed}: max |z - fp64 Box-Muller| = {err:.4e} "
          f"(allowed {4 * NORMAL_MEASURED_ERR:.4e})")
    assert err <= 4 * NORMAL_MEASURED_ERR
    # mean and std arguments: one product and one sum in fp32
    moved = _fill(C.philox_normal_, ([n], [n], [0], 0, True), torch.float32, seed, 0, 1.5, 0.25)
    assert bool(((moved.double() - (1.5 + got.double() * 0.25)).abs() <= 2.0 ** -22).all())


def _thread_tracker(seed):
    import os

    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29621")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=0, world_size=1)
    from vescale_amd.dtensor import init_device_mesh
    from vescale_amd.dtensor.random import init_rng_tracker

    mesh = init_device_mesh("cpu", (1,))
    return mesh, init_rng_tracker(mesh, "thread", seed=seed)


def _drop_tracker():
    from vescale_amd.dtensor.dispatch import get_dispatcher

    get_dispatcher()._rng_tracker = None


@requires_gpu
def test_consecutive_dropouts_are_independent():
    """Two dropout(p=0.5) in a row on a [256, 256] DTensor of ones.  For every
    lag L in -64..64 the fraction of positions with mask2[g] == mask1[g + L]
    lies within 0.5 +- 5 * 0.5 / sqrt(n - |L|), five standard deviations for
    independent masks (test_streaming_edges.py checks that streams at disjoint
    counter ranges pass this and streams 4 counters apart do not)."""
    from vescale_amd.dtensor import Replicate, distribute_tensor

    mesh, tr = _thread_tracker(777)
    try:
        x = distribute_tensor(torch.ones(256, 256, device="cuda", dtype=torch.bfloat16),
                              mesh, [Replicate()])
        tr._offset = 0
        m1 = torch.nn.functional.dropout(x, p=0.5, training=True)._local_tensor != 0
        m2 = torch.nn.functional.dropout(x, p=0.5, training=True)._local_tensor != 0
        # the first op is the offset-0 stream of the reference
        keep = sc.ref_uniform(777, 0, np.arange(256 * 256)) > np.float32(0.5)
        assert torch.equal(m1.cpu().reshape(-1), torch.from_numpy(keep))
        bad = sc.mask_agreement_violations(m1.cpu().numpy(), m2.cpu().numpy())
        assert bad == [], bad
    finally:
        _drop_tracker()


@requires_gpu
def test_consecutive_normal_fills_are_independent():
    """Two normal_ fills in a row of an fp32 [256, 256] DTensor (what deferred
    initialisation does for successive layers): at no lag in -64..64 do more
    than 2 positions hold bitwise-equal values."""
    from vescale_amd.dtensor import Replicate, distribute_tensor

    mesh, tr = _thread_tracker(778)
    try:
        tr._offset = 0
        fills = []
        for _ in range(2):
            w = distribute_tensor(torch.zeros(256, 256, device="cuda"), mesh, [Replicate()])
            w.normal_(0.0, 1.0)
            fills.append(w._local_tensor.cpu().numpy())
        assert np.isfinite(fills[0]).all() and abs(float(fills[0].std()) - 1.0) < 0.02
        count, lag = sc.max_equal_values(fills[0], fills[1])
        assert count <= 2, (count, lag)
    finally:
        _drop_tracker()
