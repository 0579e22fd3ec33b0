"""Vocab-parallel LM head + fused vocab-parallel cross-entropy against the
replicated head, one rank's work timed on ONE GPU.

    python tools/vp_ce_bench.py [--out profiles/vp_ce_ab.txt]

Shape: T = 8192 tokens, dim 4096, V = 128256, TP width w in {2, 4, 8}.
Per w, alternated inside every repetition, device-event timing:

  vp_path     head GEMM at V/w + ce_vp_fwd + ce_vp_bwd        (one rank's share)
  replicated  head GEMM at V   + dense ce_fwd + ce_bwd        (what every rank does today)
  vp_kernels / dense_kernels   the two kernel pairs alone on the SAME
              [T, V/w] tensor: equal memory traffic, the yardstick of the
              kernels themselves

The collectives of the vocab-parallel path (two all-reduces of T and 2T fp32
elements, one all-reduce of the [T, dim] activation gradient) are NOT in these
numbers: one GPU, one rank.  Bytes/s counts the algorithm's traffic (forward
reads the logits once, backward reads and writes them once: 6 bytes per
element) over the kernel pair's time, against the measured 6.29 TB/s HBM copy
rate of MI355X_MICROARCH (8.0 TB/s spec).
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

T, DIM, V = 8192, 4096, 128256
HBM_MEASURED = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--runs", type=int, default=2, help="repeat the whole measurement: spread")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import vescale_amd.ops as ops

    C = ops.require_ext()
    g = torch.Generator(device="cuda").manual_seed(0)
    h = (torch.randn(T, DIM, device="cuda", generator=g) * 0.5).bfloat16()
    w_full = (torch.randn(V, DIM, device="cuda", generator=g) * 0.02).bfloat16()
    target = torch.randint(0, V, (T,), device="cuda", generator=g)
    drow = torch.full((T,), 1.0 / T, device="cuda")
    lines = [
        "vocab-parallel head + fused vocab-parallel CE vs replicated head + dense CE",
        f"T={T} dim={DIM} V={V} bf16, {torch.cuda.get_device_name(0)}; {args.warmup} warm-up + "
        f"{args.reps} timed repetitions, sides alternated, {args.runs} runs; ms (median [min, max])",
        "one GPU, one rank: the path's collectives are NOT measured",
        "",
    ]
    for w in (2, 4, 8):
        n = V // w
        w_loc = w_full[:n].contiguous()
        t_loc = target.clamp(max=n - 1)  # dense kernels need targets inside the tensor

        def vp_kernels(x):
            picked, lse = C.ce_fwd(x, target, -100, vocab_start=0, vocab_total=V)
            return C.ce_bwd(x, target, lse, drow, -100, True, vocab_start=0, vocab_total=V)

        def dense_kernels(x, tg):
            loss, lse = C.ce_fwd(x, tg, -100)
            return C.ce_bwd(x, tg, lse, drow, -100, True)

        logits_loc = h @ w_loc.t()
        sides = {
            "vp_path": lambda: vp_kernels(h @ w_loc.t()),
            "replicated": lambda: dense_kernels(h @ w_full.t(), target),
            "vp_kernels": lambda: vp_kernels(logits_loc.clone()),
            "dense_kernels": lambda: dense_kernels(logits_loc.clone(), t_loc),
            "clone_only": lambda: logits_loc.clone(),
        }
        lines.append(f"w={w}: local shard [T, {n}]")
        meds = {k: [] for k in sides}
        for run in range(args.runs):
            times = {k: [] for k in sides}
            for rep in range(args.warmup + args.reps):
                for k, fn in sides.items():
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record()
                    out = fn()
                    t1.record()
                    torch.cuda.synchronize()
                    del out
                    if rep >= args.warmup:
                        times[k].append(t0.elapsed_time(t1))
            for k, t in times.items():
                meds[k].append(statistics.median(t))
                lines.append(f"  run {run} {k:14s} {statistics.median(t):8.3f} [{min(t):8.3f}, {max(t):8.3f}]")
        m = {k: statistics.median(v) for k, v in meds.items()}
        spread = {k: max(v) - min(v) for k, v in meds.items()}
        kv, kd = m["vp_kernels"] - m["clone_only"], m["dense_kernels"] - m["clone_only"]
        bytes_pair = 6.0 * T * n
        lines += [
            f"  one rank: vp_path {m['vp_path']:.3f} ms vs replicated {m['replicated']:.3f} ms "
            f"({m['replicated'] / m['vp_path']:.2f}x less work per rank; run-to-run spread "
            f"{spread['vp_path']:.3f} / {spread['replicated']:.3f} ms)",
            f"  same shape, kernels alone (clone of the logits subtracted): vp {kv:.3f} ms vs dense {kd:.3f} ms "
            f"(dense / vp = {kd / kv:.2f}x; run-to-run spread {spread['vp_kernels']:.3f} / "
            f"{spread['dense_kernels']:.3f} ms)",
            f"  achieved: vp {bytes_pair / kv / 1e9:.2f} TB/s, dense {bytes_pair / kd / 1e9:.2f} TB/s "
            f"of 6 B/element = {100 * bytes_pair / kv / 1e-3 / HBM_MEASURED:.0f}% / "
            f"{100 * bytes_pair / kd / 1e-3 / HBM_MEASURED:.0f}% of the measured 6.29 TB/s HBM copy rate",
            "",
        ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    sys.exit(main())
