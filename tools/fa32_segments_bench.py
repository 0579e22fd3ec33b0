"""Time of packed-document attention, forward+backward, at B4 Hq32 Hkv8 S8192
D128 causal (the method of profiles/fa_gen_segments.txt; results in
profiles/fa32_segments.txt):

    python tools/fa32_segments_bench.py [--reps 12] [--out FILE]

Run from the root of the tree whose build is to be measured (the package is
imported from the working directory), so a parent and a branch checkout can be
alternated in one session.  Variants, alternated inside every repetition:

    tuned  no ids          fa_fwd + fa_bwd2 ([B,S,H,D] o / dout, as the model runs them)
    tuned  SEG <layout>    the same with segment_ids= / seg_bounds= (pre-pass included);
                           left out on a build whose fa_fwd has no such keyword
    gen    <layout>        fa_gen_fwd + fa_gen_bwd with the same ids (its pre-passes included)

for the layouts 1 document, 8 documents of 1024 and 64 documents of 128.
Device events around the two calls, a synchronise after each; 3 warm-up and
--reps timed repetitions; median, min and max in ms.
"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())

import torch  # noqa: E402

B, HQ, HKV, S, D = 4, 32, 8, 8192, 128
LAYOUTS = (("1 doc", 1), ("8 docs of 1024", 8), ("64 docs of 128", 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: no timing without one"
    import vescale_amd.ops as ops

    ops.require_ext()
    C = ops._C
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(B, HQ, S, D, device="cuda", generator=g).bfloat16()
    k = torch.randn(B, HKV, S, D, device="cuda", generator=g).bfloat16()
    v = torch.randn(B, HKV, S, D, device="cuda", generator=g).bfloat16()
    dout = torch.randn(B, S, HQ, D, device="cuda", generator=g).bfloat16()
    dout_bhsd = dout.transpose(1, 2).contiguous()
    scale = 1.0 / math.sqrt(D)
    has_seg = "segment_ids" in (C.fa_fwd.__doc__ or "")

    def tuned(ids):
        def run():
            if ids is None:
                o, lse = C.fa_fwd(q, k, v, scale, out_bshd=True)
                return C.fa_bwd2(q, k, v, o, dout, lse, scale, False, bshd=True)
            o, lse, bounds = C.fa_fwd(q, k, v, scale, out_bshd=True, segment_ids=ids)
            return C.fa_bwd2(q, k, v, o, dout, lse, scale, False, bshd=True, seg_bounds=bounds)
        return run

    def gen(ids):
        def run():
            o, lse = C.fa_gen_fwd(q, k, v, scale, True, 0, q_seg=ids, kv_seg=ids)
            return C.fa_gen_bwd(q, k, v, o, dout_bhsd, lse, None, scale, True, 0,
                                q_seg=ids, kv_seg=ids)
        return run

    variants = [("tuned  no ids", tuned(None))]
    for name, n in LAYOUTS:
        ids = (torch.arange(S, device="cuda", dtype=torch.int32) // (S // n)).expand(B, S).contiguous()
        if has_seg:
            variants.append((f"tuned  SEG {name}", tuned(ids)))
        variants.append((f"gen    {name}", gen(ids)))

    times = {name: [] for name, _ in variants}
    for rep in range(args.warmup + args.reps):
        for name, fn in variants:
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[name].append(t0.elapsed_time(t1))
    lines = [f"{'ms per forward+backward':<28} median      min      max   ({args.reps} reps)"]
    for name, _ in variants:
        t = times[name]
        lines.append(f"{name:<28} {statistics.median(t):7.3f}  {min(t):7.3f}  {max(t):7.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
