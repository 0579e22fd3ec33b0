"""The dense wgrad layout path on the GPU: the transposing copy
(gemm_tn8 with group_form="transpose"), swiglu_packed_bwd's transposed second
output, and ops.linear with every wgrad form.

Copies are compared as int16 bit patterns.  dw is held to 2x the max abs
error of the library's own dy.t() @ x on the same inputs against an fp64 CPU
reference (another kernel sums in another order); y and dx keep F.linear's
bits."""
import pytest
import torch

import vescale_amd.ops as ops
from vescale_amd.ops import functional as VF

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")]

BF = torch.bfloat16
_SPECIAL = [0x7FC0, 0xFFC1, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x7F7F]  # NaNs, +-inf, -0.0, denormal, max


def _bits(r, c, seed):
    """[r, c] bf16 of random bit patterns with the special ones sprinkled in."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, 65536, (r * c,), generator=g, dtype=torch.int32)
    idx = torch.randint(0, r * c, (min(r * c, 63),), generator=g)
    v[idx] = torch.tensor(_SPECIAL, dtype=torch.int32).repeat(9)[: idx.numel()]
    v = torch.where(v > 32767, v - 65536, v)
    return v.to(torch.int16).reshape(r, c).cuda().view(BF)


def _eq_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16),
                                              b.contiguous().view(torch.int16))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [(8, 8), (64, 64), (72, 40), (40, 72), (264, 136)])
def test_transposing_copy_is_bitwise(shape, mode):
    x = _bits(*shape, seed=shape[0] * 1000 + shape[1])
    out = ops._C.gemm_tn8(x, [], mode, group_form="transpose")
    assert out.is_contiguous() and _eq_bits(out, x.t())


@pytest.mark.parametrize("mode", [0, 1])
def test_transposing_copy_of_a_slice(mode):
    big = _bits(3 * 128, 64, seed=7)
    x = big[128:256]  # contiguous, base 16 KiB into the allocation
    assert x.data_ptr() != big.data_ptr() and x.is_contiguous()
    keep = big.clone()
    out = ops._C.gemm_tn8(x, [], mode, group_form="transpose")
    assert _eq_bits(out, x.t()) and _eq_bits(big, keep)


@pytest.mark.parametrize("m,f", [(8, 8), (72, 40), (256, 136)])
def test_swiglu_packed_bwd_transposed_output(m, f):
    torch.manual_seed(m + f)
    dy = torch.randn(m, f, device="cuda").to(BF)
    gu = (2 * torch.randn(m, 2 * f, device="cuda")).to(BF)
    gu[0, 0], gu[-1, -1], dy[0, 0] = float("inf"), float("nan"), -0.0
    base = ops._C.swiglu_packed_bwd(dy, gu)
    dgu, dgut = ops._C.swiglu_packed_bwd(dy, gu, transposed=True)
    assert _eq_bits(dgu, base)
    assert dgut.shape == (2 * f, m) and dgut.is_contiguous() and _eq_bits(dgut, dgu.t())


LINEAR_SHAPES = [(256, 64, 128), (512, 384, 64), (520, 72, 264)]
_ref = {}


def _linear_case(m, n, k):
    """Seeded inputs, F.linear's results and the fp64 CPU dw, made once."""
    if (m, n, k) not in _ref:
        g = torch.Generator().manual_seed(m + n + k)
        x = torch.randn(2, m // 2, k, generator=g).to(BF)
        w = (torch.randn(n, k, generator=g) / k ** 0.5).to(BF)
        dy = torch.randn(2, m // 2, n, generator=g).to(BF)
        dw64 = dy.double().reshape(m, n).t() @ x.double().reshape(m, k)
        xg, wg = x.cuda().requires_grad_(), w.cuda().requires_grad_()
        y = torch.nn.functional.linear(xg, wg)
        dx, dw = torch.autograd.grad(y, (xg, wg), dy.cuda())
        err_lib = float((dw.double().cpu() - dw64).abs().max())
        _ref[(m, n, k)] = (x.cuda(), w.cuda(), dy.cuda(), dw64, y.detach(), dx, err_lib)
    return _ref[(m, n, k)]


@pytest.mark.parametrize("form", VF.WGRAD_FORMS)
@pytest.mark.parametrize("m,n,k", LINEAR_SHAPES)
def test_linear_wgrad_forms(m, n, k, form):
    x, w, dy, dw64, y_ref, dx_ref, err_lib = _linear_case(m, n, k)
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = VF.linear(xg, wg, _wgrad_form_override=form)
    assert y.grad_fn is not None and "LinearWgrad" in type(y.grad_fn).__name__
    dx, dw = torch.autograd.grad(y, (xg, wg), dy)
    assert _eq_bits(y, y_ref) and _eq_bits(dx, dx_ref)
    assert dw.shape == w.shape
    err = float((dw.double().cpu() - dw64).abs().max())
    print(f"(M,N,K)=({m},{n},{k}) form {form}: max abs err {err:.3e}, library dy.t()@x {err_lib:.3e}")
    assert err <= 2 * err_lib


def test_linear_default_rule_matches_some_form():
    """Without an override the static rule picks the form; whatever it picks,
    y and dx keep F.linear's bits and dw the bound."""
    m, n, k = LINEAR_SHAPES[0]
    x, w, dy, dw64, y_ref, dx_ref, err_lib = _linear_case(m, n, k)
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = VF.linear(xg, wg)
    dx, dw = torch.autograd.grad(y, (xg, wg), dy)
    assert _eq_bits(y, y_ref) and _eq_bits(dx, dx_ref)
    assert float((dw.double().cpu() - dw64).abs().max()) <= 2 * err_lib


@pytest.mark.parametrize("form", ["b", "c", "d"])
def test_linear_wgrad_under_graph_capture(form):
    m, n, k = LINEAR_SHAPES[0]
    x, w, dy, *_ = _linear_case(m, n, k)
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()

    def step():
        return torch.autograd.grad(VF.linear(xg, wg, _wgrad_form_override=form), (xg, wg), dy)

    eager = step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dx, dw = step()
    for _ in range(3):
        dx.fill_(7.0)
        dw.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert _eq_bits(dx, eager[0]) and _eq_bits(dw, eager[1])


def test_swiglu_hands_its_transposed_gradient_to_the_linear(monkeypatch):
    """linear (form c) -> swiglu_packed: the backward of swiglu_packed writes
    dgu^T itself, the linear transposes x only, and dw is what it is when the
    linear transposes dgu on its own.  Nothing stays attached afterwards."""
    m, n, k = LINEAR_SHAPES[0]
    x, w, *_ = _linear_case(m, n, k)
    dout = torch.randn(2, m // 2, n // 2, device="cuda").to(BF)
    calls = []
    real = VF._transposed
    monkeypatch.setattr(VF, "_transposed", lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    results = []
    for channel in (True, False):
        calls.clear()
        xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = VF.linear(xg, wg, _wgrad_form_override="c")
        assert getattr(y, VF._WGRAD_WANTS_T) is True
        if not channel:
            delattr(y, VF._WGRAD_WANTS_T)
        seen = []
        y.register_hook(lambda g: seen.append(g))
        dx, dw = torch.autograd.grad(VF.swiglu_packed(y), (xg, wg), dout)
        assert calls == ([(m, k)] if channel else [(m, n), (m, k)])
        assert not hasattr(seen[0], VF._WGRAD_T)
        results.append((dx, dw))
    assert _eq_bits(results[0][0], results[1][0]) and _eq_bits(results[0][1], results[1][1])


def test_w13_wgrad_keeps_the_bits_of_the_library_call():
    """The one shape the static rule moves to form (c) in the flagship model
    (Llama-3-8B w13 at 4 x 8192 tokens): a training run reproduces the run
    before the change only if dw keeps its bits there, i.e. if the library's
    kernel for dyT @ xT.t() sums in the order of its kernel for dy.t() @ x.
    About 2 x 7.7 TFLOP and 4.5 GB; the shape is the point of the test."""
    m, n, k = 32768, 28672, 4096
    assert VF._wgrad_form(m, n, k) == "c"
    g = torch.Generator(device="cuda").manual_seed(5)
    dy = torch.randn(m, n, device="cuda", generator=g).mul_(1e-3).to(BF)
    x = torch.randn(m, k, device="cuda", generator=g).to(BF)
    want = dy.t() @ x
    got = VF._transposed(dy) @ VF._transposed(x).t()
    assert _eq_bits(got, want)
