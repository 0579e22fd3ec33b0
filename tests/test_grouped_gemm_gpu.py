"""Grouped expert GEMM (gemm_tn8 with group_form) against a per-group fp64
matmul of the same bf16 inputs.  Bound, elementwise: |out - ref| <= 2^-8 |ref|
+ K_c 2^-23 (|A| . |B|^T), K_c the contraction length.  Operands sit between 256
NaN rows on either side, weights are separate tensors, outputs start as a sentinel."""
import pytest
import torch

import vescale_amd.ops as ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")]

E = 4
SHAPES = [(128, 128), (384, 256)]
OFFSETS = [[0, 0, 1, 130, 130], [0, 128, 256, 256, 300], [0, 0, 0, 0, 77], [0, 0, 0, 0, 0]]
SENTINEL, BF = 7.0, torch.bfloat16


def _inputs(K, N, T):
    torch.manual_seed(K + N + T)
    guarded = []
    for cols in (K, N):
        buf = torch.full((T + 512, cols), float("nan"), device="cuda", dtype=BF)
        buf[256:256 + T] = torch.randn(T, cols, device="cuda")
        guarded.append(buf[256:256 + T])
    return (*guarded, [torch.randn(N, K, device="cuda").to(BF) for _ in range(E)])


def _groups(offs, T):  # the kernels' rule: clamp to [0, T], then a running maximum
    b = torch.tensor(offs).clamp(0, T).cummax(0)[0].tolist()
    return list(zip(b[:-1], b[1:]))


def _run(form, x, dy, ws, offs):
    o = torch.tensor(offs, dtype=torch.int32, device="cuda")
    T, (N, K) = x.shape[0], ws[0].shape
    shape = {"fwd": (T, N), "dgrad": (T, K), "wgrad": (E, N, K)}[form]
    out = torch.full(shape, SENTINEL, device="cuda", dtype=BF)
    kw = dict(group_x=x) if form == "wgrad" else {}
    return ops._C.gemm_tn8(x if form == "fwd" else dy, ws, 0, group_offsets=o, group_form=form,
                           group_out=out, **kw)


def _check(form, out, x, dy, ws, offs):
    assert torch.isfinite(out).all(), form
    covered = torch.zeros(x.shape[0], dtype=torch.bool, device="cuda")
    for e, (lo, hi) in enumerate(_groups(offs, x.shape[0])):
        covered[lo:hi] = True
        xe, de, w = x[lo:hi].double(), dy[lo:hi].double(), ws[e].double()
        if form == "fwd":
            got, a, b, kc = out[lo:hi], xe, w.t(), x.shape[1]
        elif form == "dgrad":
            got, a, b, kc = out[lo:hi], de, w, dy.shape[1]
        else:
            got, a, b, kc = out[e], de.t(), xe, hi - lo
            if hi == lo:
                assert (got == 0).all(), f"empty group {e}: dW must be exactly zero"
        ref = a @ b
        bound = 2.0 ** -8 * ref.abs() + kc * 2.0 ** -23 * (a.abs() @ b.abs())
        err = (got.double() - ref).abs()
        assert (err <= bound).all(), (form, e, float((err - bound).max()))
    if form != "wgrad":
        assert (out[~covered] == SENTINEL).all(), f"{form}: a row outside the groups was written"


@pytest.mark.parametrize("offs", OFFSETS)
@pytest.mark.parametrize("K,N", SHAPES)
def test_binding_forms(K, N, offs):
    x, dy, ws = _inputs(K, N, offs[-1])
    for form in ("fwd", "dgrad", "wgrad"):
        out = _run(form, x, dy, ws, offs)
        _check(form, out, x, dy, ws, offs)
        assert torch.equal(out.view(torch.int16), _run(form, x, dy, ws, offs).view(torch.int16)), \
            f"{form}: two calls differ in their bits"
        if form != "wgrad":  # one stacked [E,N,K] tensor reads the same weights
            assert torch.equal(out, _run(form, x, dy, torch.stack(ws), offs))


@pytest.mark.parametrize("offs", OFFSETS)
@pytest.mark.parametrize("K,N", SHAPES)
def test_grouped_linear_backward(K, N, offs):
    x, dy, ws = _inputs(K, N, offs[-1])
    xr, *wr = (t.detach().requires_grad_() for t in (x, *ws))
    y = ops.grouped_linear(xr, wr, torch.tensor(offs, dtype=torch.int32, device="cuda"))
    y.backward(dy)
    _check("fwd", y.detach(), x, dy, ws, offs)
    _check("dgrad", xr.grad, x, dy, ws, offs)
    _check("wgrad", torch.stack([w.grad for w in wr]), x, dy, ws, offs)


def test_hostile_offsets():  # clamped and monotone: the groups [0,200), {}, {}, {}; run once
    offs = [0, 500, 3, -7, 10 ** 6]
    x, dy, ws = _inputs(128, 128, 200)
    for form in ("fwd", "dgrad", "wgrad"):
        _check(form, _run(form, x, dy, ws, offs), x, dy, ws, offs)
