"""fa_gen_fwd + fa_gen_bwd at B4 Hq32 Hkv8 S8192 D128 causal with a window
(profiles/fa_gen_window.txt): windows (1023, 0) and (4095, 0) against no
window on this build and, with --parent-ext PATH (the extension module built
from the commit before the window), no window on this build against that
build.  The variants of a comparison alternate sample by sample; device
events around the two calls, a synchronise after each.

    python tools/fa_gen_window_bench.py [--samples 30] [--parent-ext PATH]
"""
import argparse
import importlib.util
import statistics

import torch

import vescale_amd.ops as ops

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=30)
ap.add_argument("--parent-ext", default=None)
args = ap.parse_args()
N = args.samples


def load(path):
    spec = importlib.util.spec_from_file_location("_C", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


ops.require_ext()
branch = ops.functional._ext()
parent = load(args.parent_ext) if args.parent_ext else None

B, Hq, Hkv, S, D = 4, 32, 8, 8192, 128
g = torch.Generator(device="cuda").manual_seed(0)
q = torch.randn(B, Hq, S, D, device="cuda", generator=g).bfloat16()
k = torch.randn(B, Hkv, S, D, device="cuda", generator=g).bfloat16()
v = torch.randn(B, Hkv, S, D, device="cuda", generator=g).bfloat16()
dout = torch.randn(B, Hq, S, D, device="cuda", generator=g).bfloat16()
scale = D ** -0.5

def call(ext, lower):
    kw = {} if lower is None else {"lower": lower}
    o, lse = ext.fa_gen_fwd(q, k, v, scale, True, 0, **kw)
    dq, dk, dv = ext.fa_gen_bwd(q, k, v, o, dout, lse, None, scale, True, 0, **kw)
    return o, lse, dq, dk, dv

def sample(ext, lower):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); call(ext, lower); b.record(); b.synchronize()
    return a.elapsed_time(b)

def alternate(variants, n):
    for _ in range(3):
        for e, l in variants.values(): sample(e, l)
    t = {name: [] for name in variants}
    for _ in range(n):
        for name, (e, l) in variants.items(): t[name].append(sample(e, l))
    return t

def share(left):
    """visited (q tile, kv tile) pairs over the causal pairs, fwd/dq ranges"""
    nt = S // 64
    full = sum(i + 1 for i in range(nt))
    vis = sum(i + 1 - max(0, i * 64 - left) // 64 for i in range(nt))
    return vis / full

lines = []
def report(title, t):
    lines.append(title)
    for name, xs in t.items():
        med = statistics.median(xs)
        lines.append(f"  {name:28s} median {med:8.3f} ms  min {min(xs):8.3f}  max {max(xs):8.3f}"
                     f"  spread {max(xs) - min(xs):6.3f} ms ({100 * (max(xs) - min(xs)) / med:.2f}%)  n={len(xs)}")

if parent is not None:
    # results first: the non-window path must compute what the parent computes
    rp, rb = call(parent, None), call(branch, None)
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(rp, rb))
    lines.append(f"no window, parent vs this build, o/lse/dq/dk/dv bitwise equal: {same}")
    report("1) no window: parent build vs this build, alternating",
           alternate({"parent": (parent, None), "this build": (branch, None)}, N))
t = alternate({"no window": (branch, None), "window (1023, 0)": (branch, -1023),
               "window (4095, 0)": (branch, -4095)}, N)
report("2) this build: windows vs no window, alternating", t)
base = statistics.median(t["no window"])
for name, left in (("window (1023, 0)", 1023), ("window (4095, 0)", 4095)):
    med = statistics.median(t[name])
    lines.append(f"  {name}: {med / base:.3f}x of no window; tile pairs visited {share(left):.3f} of the causal ones")
print("\n".join(lines))
