"""CPU tier of the dense-GEMM tests: the cases of tests/gemm_cases.py keep
their oracles exact, and a correct GEMM meets the rounding bound.  Nothing here
runs a HIP kernel; test_gemm_dense_gpu.py does, at the same cases.

Every check is a large matmul, which warms torch's thread pool.  Doing that in
the pytest parent makes the forked multi-process tests that run later hang
(tests/README.md, fork-safety rule), so all checks run in ONE child process
and each test reads its own line of the child's report."""
import os
import subprocess
import sys
import traceback

import pytest

from tests import gemm_cases as gc


# ---------------------------------------------------------------------------
# the checks (run in the child)
# ---------------------------------------------------------------------------
def _check_exact(M, N, K):
    """For every exact case the GPU tier launches: the fp32 product of the
    same operands, summed in whatever order the CPU library picks, equals the
    fp64 one, and |C| stays below 2^24.  This proves the inputs, not a kernel:
    any fp32 accumulation order gives the integers of the true product."""
    import torch

    a, b = gc.exact_case(M, N, K)
    for t in (a, b):
        assert t.dtype == torch.bfloat16
        assert torch.equal(t.float(), t.float().round()) and t.float().abs().max() <= 4
    ref = gc.product64(a, b)
    assert ref.abs().max().item() < 2 ** 24
    assert torch.equal((a.float() @ b.float().t()).double(), ref)
    # and the bf16 rounding of those integers is not the identity at this K:
    # the comparison exercises round-to-nearest-even, not only small sums
    if K >= 1024:
        assert not torch.equal(ref.float().bfloat16().double(), ref)


def _check_one_chunk():
    """One lost, repeated or stale 8-element chunk changes the expected
    result: dropping k = 8..15 of one row of a, or reading them twice, moves
    that row of C by an integer that survives the bf16 rounding."""
    import torch

    a, b = gc.exact_case(256, 256, 128)
    want = gc.exact_expected(a, b)
    lost = a.clone()
    lost[5, 8:16] = 0
    twice = a.clone()
    twice[5, 16:24] = a[5, 8:16]
    for other in (lost, twice):
        got = gc.product64(other, b).float().bfloat16()
        assert not torch.equal(got[5], want[5])
        try:
            gc.assert_exact(got, a, b, "chunk")
        except AssertionError as e:
            assert "first at [5, " in str(e), e
        else:
            raise AssertionError("assert_exact accepted a result with a chunk missing")


def _check_placement(M, N, K):
    import torch

    a, b = gc.placement_case(M, N, K)
    c = gc.exact_expected(a, b).double()
    i, j = torch.arange(M)[:, None], torch.arange(N)[None, :]
    assert torch.equal(c, ((j % 7) - 3 + ((i % K) % 5)).double())
    assert not torch.equal(b[:K, :K], b[:K, :K].t())
    # neighbouring tile rows and tile columns differ, so a tile written to the
    # wrong place is seen
    for bm, bn in {(v[0], v[1]) for v in gc.TN_VARIANTS.values()}:
        if M > bm and M % bm == 0 and N > bn and N % bn == 0:
            assert not torch.equal(c[:bm], c[bm:2 * bm])
            assert not torch.equal(c[:, :bn], c[:, bn:2 * bn])


def _check_rounding(M, N, K):
    """A plain bf16 torch.matmul on the CPU meets the bound, and the bound is
    no blank cheque: with one 8-element chunk of one row of a left out, most
    of that row of the result misses it."""
    import torch

    a, b = gc.rounding_case(M, N, K)
    got = a @ b.t()
    assert got.dtype == torch.bfloat16
    gc.assert_within_rounding(got, a, b, f"cpu bf16 matmul {M}x{N}x{K}")
    ref, bound = gc.rounding_bound(a, b)
    lost = a.clone()
    lost[5, 8:16] = 0
    frac = (((lost @ b.t()).double() - ref).abs() > bound)[5].double().mean().item()
    assert frac > 0.5, frac


def _check_linear8(name):
    """The fp64 autograd oracle and its three bounds admit the plain bf16
    linear of the CPU."""
    import torch

    x, w, dy = gc.linear8_case(name)
    (y, dx, dw), (by, bdx, bdw) = gc.linear8_oracle(x, w, dy)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    yr = torch.nn.functional.linear(xr, wr)
    yr.backward(dy)
    for got, ref, bound in ((yr.detach(), y, by), (xr.grad, dx, bdx), (wr.grad, dw, bdw)):
        assert got.shape == ref.shape == bound.shape
        assert bool(((got.double() - ref).abs() <= bound).all()), name


def _checks():
    """(id, function, arguments) of every check, in a fixed order."""
    out = [(f"exact-{M}x{N}x{K}", _check_exact, (M, N, K)) for M, N, K in gc.all_exact_shapes()]
    out.append(("one-chunk", _check_one_chunk, ()))
    out += [(f"placement-{M}x{N}x{K}", _check_placement, (M, N, K))
            for M, N, K in gc.placement_shapes()]
    out += [(f"rounding-{M}x{N}x{K}", _check_rounding, (M, N, K))
            for M, N, K in [(64, 96, 160), gc.ROUNDING_SHAPE]]
    out += [(f"linear8-{name}", _check_linear8, (name,)) for name in gc.LINEAR8_CASES]
    return out


def _run_all():
    """The child's body: one report line per check."""
    for cid, fn, args in _checks():
        try:
            fn(*args)
            print(f"CHECK\t{cid}\tOK", flush=True)
        except Exception:  # noqa: BLE001 - reported to the parent, which fails the test
            text = traceback.format_exc().strip().replace("\n", " | ")
            print(f"CHECK\t{cid}\tFAIL {text}", flush=True)


# ---------------------------------------------------------------------------
# the tests (read the child's report)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); "
            "from tests.test_gemm_dense import _run_all; _run_all()") % root
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-1500:]
    lines = {}
    for ln in out.stdout.splitlines():
        if ln.startswith("CHECK\t"):
            _, cid, verdict = ln.split("\t", 2)
            lines[cid] = verdict
    return lines


@pytest.mark.parametrize("cid", [c[0] for c in _checks()])
def test_gemm_oracle(report, cid):
    """See the _check_* function that the id names."""
    assert report.get(cid, "did not run") == "OK"
