"""Dense wgrad GEMM by operand layout, and the transposing copy that buys it.

    python tools/wgrad_layout_ab.py [--out-dir profiles] [--window 1.0]
    python tools/wgrad_layout_ab.py --names          # under rocprofv3 --kernel-trace
    python tools/wgrad_layout_ab.py --parse-trace X_kernel_trace.csv

dw [N,K] = dy^T . x at M = 32768 for the four layer shapes of Llama-3-8B and
the LM head, through torch.matmul in the four forms of ops.functional
(WGRAD_FORMS): (a) dy.t() @ x, (b) dyT @ x, (c) dyT @ xT.t(), (d) xT @ dy
(= dw^T).  Every form is timed with device events over a window of at least
--window seconds of back-to-back calls (short windows run at boost clocks),
the forms alternating, every form twice.  The transposes a form needs are
timed the same way and listed beside it; nothing is added up silently.

Second table: the transposing copy (both tiles) against torch's copy_ of the
same bytes and against x.t().contiguous(), and swiglu_packed_bwd with and
without its transposed output.

--names runs every (shape, form) product three times, in the order it prints,
with nothing in between; --parse-trace reads the kernel trace of that run and
prints the library kernel of every form (the Cijk_* / Custom_Cijk_* names,
in groups of three).  No GPU: the tool fails, it does not fall back.
"""
from __future__ import annotations

import argparse
import csv
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M = 32768
SHAPES = [  # (N, K), layer
    ((6144, 4096), "qkv"),
    ((4096, 4096), "wo"),
    ((28672, 4096), "w13"),
    ((4096, 14336), "w2"),
    ((128256, 4096), "head"),
]
FORMS = ("a", "b", "c", "d")


def products(dy, x, dyT, xT):
    return {
        "a": lambda: dy.t() @ x,
        "b": lambda: dyT @ x,
        "c": lambda: dyT @ xT.t(),
        "d": lambda: xT @ dy,
    }


def window_ms(fn, window_s):
    """Mean ms per call over >= window_s of back-to-back calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(3, int(window_s * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps


def operands(n, k):
    g = torch.Generator(device="cuda").manual_seed(n + k)
    dy = torch.randn(M, n, device="cuda", dtype=torch.bfloat16, generator=g)
    x = torch.randn(M, k, device="cuda", dtype=torch.bfloat16, generator=g)
    return dy, x, dy.t().contiguous(), x.t().contiguous()


def layout_table(window_s, out):
    from vescale_amd.ops.functional import _transposed

    out.append(f"# dw[N,K] = dy^T . x, M = {M}, bf16, torch.matmul; ms per call, mean over a "
               f">= {window_s} s window, two windows per form (forms alternating)")
    out.append("# T(dy), T(x), T(dwT): the transposing copy of that operand (transpose.hip)")
    out.append(f"{'layer':5} {'N':>6} {'K':>6} {'TF':>6} | " +
               " | ".join(f"({f}) r1    r2   PF/s" for f in FORMS) +
               " | T(dy)  T(x)  T(dwT)")
    for (n, k), layer in SHAPES:
        dy, x, dyT, xT = operands(n, k)
        fns = products(dy, x, dyT, xT)
        ms = {f: [] for f in FORMS}
        for _ in range(2):
            for f in FORMS:
                ms[f].append(window_ms(fns[f], window_s)[0])
        dwT = fns["d"]()
        t_dy = window_ms(lambda: _transposed(dy), 0.3)[0]
        t_x = window_ms(lambda: _transposed(x), 0.3)[0]
        t_dw = window_ms(lambda: _transposed(dwT), 0.3)[0]
        tf = 2.0 * M * n * k / 1e12
        cells = " | ".join(
            f"{ms[f][0]:7.3f} {ms[f][1]:7.3f} {tf / min(ms[f]):5.2f}" for f in FORMS)
        out.append(f"{layer:5} {n:6d} {k:6d} {tf:6.2f} | {cells} | {t_dy:5.3f} {t_x:5.3f} {t_dw:5.3f}")
        print(out[-1], flush=True)
        del dy, x, dyT, xT, dwT, fns
        torch.cuda.empty_cache()


def transposed_table(out):
    import vescale_amd.ops as ops

    ext = ops.require_ext()
    out.append("# transposing copy [R,C] -> [C,R] bf16: ms per call and TB/s (read + write), "
               ">= 0.5 s windows")
    out.append(f"{'R':>6} {'C':>6} | {'copy_':>14} | {'tile 64':>14} | {'tile 128':>14} | "
               f"{'t().contiguous()':>16} | tile64/copy tile128/copy")
    for r, c in ((32768, 4096), (32768, 14336), (32768, 28672)):
        x = torch.randn(r, c, device="cuda", dtype=torch.bfloat16)
        dst = torch.empty_like(x)
        gb = 2 * x.numel() * 2 / 1e9
        t_copy = window_ms(lambda: dst.copy_(x), 0.5)[0]
        t64 = window_ms(lambda: ext.gemm_tn8(x, [], 1, group_form="transpose"), 0.5)[0]
        t128 = window_ms(lambda: ext.gemm_tn8(x, [], 0, group_form="transpose"), 0.5)[0]
        t_torch = window_ms(lambda: x.t().contiguous(), 0.5)[0]
        cell = lambda t: f"{t:6.3f} {gb / t:6.2f}"
        out.append(f"{r:6d} {c:6d} | {cell(t_copy)} | {cell(t64)} | {cell(t128)} | "
                   f"{cell(t_torch):>16} | {t_copy / t64:6.3f} {t_copy / t128:6.3f}")
        print(out[-1], flush=True)
        del x, dst
    f = 14336
    dy = torch.randn(M, f, device="cuda", dtype=torch.bfloat16)
    gu = torch.randn(M, 2 * f, device="cuda", dtype=torch.bfloat16)
    t0 = window_ms(lambda: ext.swiglu_packed_bwd(dy, gu), 0.5)[0]
    t1 = window_ms(lambda: ext.swiglu_packed_bwd(dy, gu, transposed=True), 0.5)[0]
    out.append(f"# swiglu_packed_bwd [{M},{f}]: {t0:.3f} ms ({dy.numel() * 2 * 5 / 1e9 / t0:.2f} TB/s); "
               f"with the transposed output {t1:.3f} ms ({dy.numel() * 2 * 7 / 1e9 / t1:.2f} TB/s)")
    print(out[-1], flush=True)


def run_names():
    for (n, k), layer in SHAPES:
        dy, x, dyT, xT = operands(n, k)
        fns = products(dy, x, dyT, xT)
        for f in FORMS:
            for _ in range(3):
                fns[f]()
            print(f"{layer} ({f}) x3", flush=True)
        torch.cuda.synchronize()
        del dy, x, dyT, xT, fns
        torch.cuda.empty_cache()


def parse_trace(path):
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows
             if r["Kernel_Name"].startswith(("Cijk_", "Custom_Cijk_"))]
    want = 3 * len(FORMS) * len(SHAPES)
    if len(names) != want:
        print(f"# {len(names)} library GEMM dispatches, expected {want}: raw order follows")
        for nm in names:
            print(nm)
        return
    it = iter(names)
    for (n, k), layer in SHAPES:
        for f in FORMS:
            trio = {next(it) for _ in range(3)}
            print(f"{layer:5} ({f}) {' / '.join(sorted(trio))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default="profiles")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--names", action="store_true")
    ap.add_argument("--parse-trace")
    args = ap.parse_args()
    if args.parse_trace:
        return parse_trace(args.parse_trace)
    if not torch.cuda.is_available():
        raise SystemExit("wgrad_layout_ab needs a GPU")
    if args.names:
        return run_names()
    os.makedirs(args.out_dir, exist_ok=True)
    out = []
    transposed_table(out)
    with open(os.path.join(args.out_dir, "wgrad_transposed_ab.txt"), "w") as fh:
        fh.write("\n".join(out) + "\n")
    out = []
    layout_table(args.window, out)
    with open(os.path.join(args.out_dir, "wgrad_layout_ab.txt"), "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
