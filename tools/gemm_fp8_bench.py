"""The fp8 GEMM, its quantiser kernels and the fp8 linear (VESCALE_GEMM=fp8)
against the default bf16 library path, at the Llama-3-8B linear shapes with
M = 32768 tokens (profiles/gemm_fp8_ab.txt):

  per shape (wqkv, wo, w13, w2), alternating sample by sample:
    1) the three products alone (forward, dgrad, wgrad): the fp8 GEMM on
       already quantised operands vs the bf16 library product in the layout
       F.linear and its autograd issue, and, where this torch has it,
       torch._scaled_mm on the same fp8 operands
    2) the amax and the cast (q and q^T) kernels alone on x [M,K]
    3) linear() forward + backward end to end: fp8 vs the default backend

Device events around each sample, a synchronise after it, three warm-up
rounds; median, min, max and spread are printed.  One GPU.

    python tools/gemm_fp8_bench.py [--samples 10] [--m 32768]
"""
import argparse
import os
import statistics

import torch

import vescale_amd.ops as ops
from vescale_amd.ops.functional import _fp8_quantize

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=10)
ap.add_argument("--m", type=int, default=32768)
args = ap.parse_args()

C = ops.require_ext()
M = args.m
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
SHAPES = {"wqkv": (6144, 4096), "wo": (4096, 4096), "w13": (28672, 4096), "w2": (4096, 14336)}
g = torch.Generator(device="cuda").manual_seed(0)
has_scaled_mm = hasattr(torch, "_scaled_mm")


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, n):
    for _ in range(3):
        for fn in variants.values(): sample(fn)
    t = {name: [] for name in variants}
    for _ in range(n):
        for name, fn in variants.items(): t[name].append(sample(fn))
    return t


def report(title, t, flop=None):
    print(title)
    for name, xs in t.items():
        med = statistics.median(xs)
        rate = f"  {flop / med / 1e9:7.1f} TF/s" if flop else ""
        print(f"  {name:34s} median {med:8.3f} ms  min {min(xs):8.3f}  max {max(xs):8.3f}"
              f"  spread {max(xs) - min(xs):6.3f} ms ({100 * (max(xs) - min(xs)) / med:.2f}%){rate}"
              f"  n={len(xs)}", flush=True)


def products(aq, sa, bq, sb, lib):
    """variants of one TN product aq [m,k] . bq [n,k]^T; lib() is the bf16
    library call of the same product."""
    v = {"fp8 GEMM (gemm_fp8.hip)": lambda: C.gemm_tn8(aq, bq, 0, scale_a=sa, scale_b=sb),
         "bf16 library": lib}
    if has_scaled_mm:
        mm = lambda: torch._scaled_mm(aq, bq.t(), scale_a=sa, scale_b=sb,  # noqa: E731
                                      out_dtype=torch.bfloat16)
        try:
            mm()
            torch.cuda.synchronize()
            v["torch._scaled_mm"] = mm
        except Exception as e:  # not every dtype pair or shape has a library kernel
            print(f"  (torch._scaled_mm left out: {str(e).splitlines()[0][:100]})")
    return v


def linear(backend, x, w, dy):
    def run():
        os.environ["VESCALE_GEMM"] = backend
        y = ops.linear(x, w)
        torch.autograd.grad(y, [x, w], dy)
    return run


print(f"M = {M}, samples = {args.samples}, torch._scaled_mm: {has_scaled_mm}")
for name, (N, K) in SHAPES.items():
    x = torch.randn(M, K, device="cuda", generator=g).bfloat16().requires_grad_(True)
    w = (torch.randn(N, K, device="cuda", generator=g) / 64).bfloat16().requires_grad_(True)
    dy = torch.randn(M, N, device="cuda", generator=g).bfloat16()
    with torch.no_grad():
        xq, xqt, sx = _fp8_quantize(x, E4M3)
        wq, wqt, sw = _fp8_quantize(w, E4M3)
        dyq, dyqt, sd = _fp8_quantize(dy, E5M2)
        flop = 2.0 * M * N * K
        print(f"== {name}: x [{M},{K}], w [{N},{K}]")
        report("1a) forward  y = x w^T", alternate(
            products(xq, sx, wq, sw, lambda: torch.nn.functional.linear(x, w)),
            args.samples), flop)
        report("1b) dgrad    dx = dy w", alternate(
            products(dyq, sd, wqt, sw, lambda: dy @ w), args.samples), flop)
        report("1c) wgrad    dw = dy^T x", alternate(
            products(dyqt, sd, xqt, sx, lambda: dy.t() @ x), args.samples), flop)
        q, qt = torch.empty_like(xq), torch.empty_like(xqt)
        report("2) quantiser kernels on x", alternate({
            "fp8_amax": lambda: C.gemm_tn8(x, [], 0, group_form="fp8_amax"),
            "fp8_quantize (q and q^T)": lambda: C.gemm_tn8(
                x, [], 0, group_form="fp8_quantize", scale_a=sx, group_out=q, out_t=qt),
            "fp8_quantize (q only)": lambda: C.gemm_tn8(
                x, [], 0, group_form="fp8_quantize", scale_a=sx, group_out=q),
        }, args.samples))
        del xq, xqt, wq, wqt, dyq, dyqt, q, qt
    report("3) linear() forward + backward", alternate(
        {"VESCALE_GEMM=fp8": linear("fp8", x, w, dy),
         "VESCALE_GEMM=blaslt (default)": linear("blaslt", x, w, dy)}, args.samples), 3 * flop)
    del x, w, dy
