"""The tuned 32x32 flash kernels beyond causal self-attention, forward plus
backward through flash_attention at B4 Hq32 Hkv8 D128 (profiles/fa32_full.txt):

  1) S8192 non-causal: tuned (FULL kernels) vs general (VESCALE_FA_FULL=gen)
     vs F.scaled_dot_product_attention
  2) a ring-shaped set on one GPU, S_local 2048: one causal block and three
     non-causal blocks, each with return_lse, merged as ring_sdpa merges, and
     a backward through the merge: tuned vs general
  3) S8192 causal with return_lse: tuned vs general; and the causal no-lse
     path (fa_fwd + fa_bwd2, as _FlashAttention calls them) on this build
     against, with --parent-ext PATH, the extension built from the commit before

The variants of a comparison alternate sample by sample; device events around
each sample, a synchronise after it.  One GPU; no multi-GPU ring is run.

    python tools/fa_full_bench.py [--samples 20] [--parent-ext PATH]
"""
import argparse
import importlib.util
import os
import statistics

import torch
import torch.nn.functional as F

import vescale_amd.ops as ops
from vescale_amd.dmodule.ring_attention import _merge
from vescale_amd.ops import flash_attention

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=20)
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

B, Hq, Hkv, D = 4, 32, 8, 128
scale = D ** -0.5
g = torch.Generator(device="cuda").manual_seed(0)


def inputs(S):
    r = lambda h: torch.randn(B, h, S, D, device="cuda", generator=g).bfloat16()
    return r(Hq).requires_grad_(True), r(Hkv).requires_grad_(True), r(Hkv).requires_grad_(True), r(Hq)


def flash(backend, causal, lse):
    """forward + backward of one flash_attention call on `backend`."""
    def run(q, k, v, dout):
        os.environ["VESCALE_FA_FULL"] = backend
        r = flash_attention(q, k, v, is_causal=causal, return_lse=lse)
        o = r[0] if lse else r
        torch.autograd.grad(o, [q, k, v], dout)
    return run


def sdpa(q, k, v, dout):
    o = F.scaled_dot_product_attention(q, k, v, is_causal=False, enable_gqa=True)
    torch.autograd.grad(o, [q, k, v], dout)


def ring(backend):
    """What one rank of a 4-way causal ring computes: its diagonal block and
    three past blocks (here the same k/v four times), merged, then backward."""
    def run(q, k, v, dout):
        os.environ["VESCALE_FA_FULL"] = backend
        acc = lse = None
        for step in range(4):
            o, l = flash_attention(q, k, v, is_causal=step == 0, return_lse=True)
            o, l = o.float(), l.unsqueeze(-1)
            acc, lse = (o, l) if step == 0 else _merge(acc, lse, o, l)
        torch.autograd.grad(acc.to(torch.bfloat16), [q, k, v], dout)
    return run


def causal_ext(ext):
    def run(q, k, v, dout):
        o, lse = ext.fa_fwd(q, k, v, scale, out_bshd=True)
        ext.fa_bwd2(q, k, v, o, dout_t, lse, scale, False, bshd=True)
    return run


def sample(fn, xs):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(*xs); b.record(); b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, xs, n):
    for _ in range(3):
        for fn in variants.values(): sample(fn, xs)
    t = {name: [] for name in variants}
    for _ in range(n):
        for name, fn in variants.items(): t[name].append(sample(fn, xs))
    return t


def report(title, t):
    print(title)
    for name, xs in t.items():
        med = statistics.median(xs)
        print(f"  {name:30s} median {med:8.3f} ms  min {min(xs):8.3f}  max {max(xs):8.3f}"
              f"  spread {max(xs) - min(xs):6.3f} ms ({100 * (max(xs) - min(xs)) / med:.2f}%)  n={len(xs)}",
              flush=True)


xs = inputs(8192)
report("1) S8192 non-causal, fwd + bwd, alternating",
       alternate({"tuned (FULL)": flash("tuned", False, False),
                  "general (VESCALE_FA_FULL=gen)": flash("gen", False, False),
                  "F.scaled_dot_product_attention": sdpa}, xs, N))
report("3a) S8192 causal, return_lse, fwd + bwd, alternating",
       alternate({"tuned (causal kernels + lse)": flash("tuned", True, True),
                  "general (VESCALE_FA_FULL=gen)": flash("gen", True, True)}, xs, N))
q, k, v, dout = (t.detach() for t in xs)
dout_t = dout.transpose(1, 2).contiguous()
variants = {"this build": causal_ext(branch)}
if parent is not None:
    rp = parent.fa_fwd(q, k, v, scale, out_bshd=True)
    rp += parent.fa_bwd2(q, k, v, rp[0], dout_t, rp[1], scale, False, bshd=True)
    rb = branch.fa_fwd(q, k, v, scale, out_bshd=True)
    rb += branch.fa_bwd2(q, k, v, rb[0], dout_t, rb[1], scale, False, bshd=True)
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(rp, rb))
    print(f"causal no-lse, parent vs this build, o/lse/dq/dk/dv bitwise equal: {same}")
    variants = {"parent build": causal_ext(parent), **variants}
report("3b) S8192 causal, no lse (fa_fwd + fa_bwd2, [B,S,H,D] o/dout), alternating",
       alternate(variants, (q, k, v, dout), N))
del xs, q, k, v, dout, dout_t
report("2) ring-shaped set, S_local 2048: 1 causal + 3 non-causal blocks with lse, merge, bwd",
       alternate({"tuned": ring("tuned"), "general (VESCALE_FA_FULL=gen)": ring("gen")},
                 inputs(2048), N))
