"""Forward+backward time of the general flash attention kernel
(ops.flash_attention -> attention_gen.hip) against
F.scaled_dot_product_attention at shapes the tuned D=128 kernels reject.

    python tools/fa_gen_bench.py [--out profiles/fa_gen_vs_sdpa.txt]

Device-event timing, warm-up, the two sides alternated inside every
repetition; reports median / min / max over the timed repetitions and the
largest output difference between the two sides.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

# name, B, Hq, Hkv, S, D, causal
SHAPES = [
    ("B4 Hq32 Hkv8 S4160 D128 causal", 4, 32, 8, 4160, 128, True),
    ("B4 H12 S1000 D64 non-causal", 4, 12, 12, 1000, 64, False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from vescale_amd.ops import flash_attention

    lines = [
        "general flash attention kernel vs F.scaled_dot_product_attention",
        f"forward+backward, bf16, {torch.cuda.get_device_name(0)}; "
        f"{args.warmup} warm-up + {args.reps} timed repetitions, sides alternated; ms",
        "",
    ]
    for name, B, Hq, Hkv, S, D, causal in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        mk = lambda h: torch.randn(B, h, S, D, device="cuda", generator=g).bfloat16().requires_grad_(True)
        q, k, v = mk(Hq), mk(Hkv), mk(Hkv)
        dout = torch.randn(B, Hq, S, D, device="cuda", generator=g).bfloat16()
        sides = {
            "fa_gen": lambda: flash_attention(q, k, v, is_causal=causal),
            "sdpa": lambda: F.scaled_dot_product_attention(
                q, k, v, is_causal=causal, enable_gqa=Hq != Hkv),
        }
        times = {n: [] for n in sides}
        outs = {}
        for rep in range(args.warmup + args.reps):
            for n, fn in sides.items():
                t0 = torch.cuda.Event(enable_timing=True)
                t1 = torch.cuda.Event(enable_timing=True)
                t0.record()
                out = fn()
                torch.autograd.grad(out, [q, k, v], dout)
                t1.record()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    times[n].append(t0.elapsed_time(t1))
                outs[n] = out.detach()
        diff = (outs["fa_gen"].float() - outs["sdpa"].float()).abs().max().item()
        med = {n: statistics.median(t) for n, t in times.items()}
        lines.append(name)
        for n, t in times.items():
            lines.append(f"  {n:7s} median {med[n]:8.3f}  min {min(t):8.3f}  max {max(t):8.3f}")
        winner = min(med, key=med.get)
        ratio = med["fa_gen"] / med["sdpa"]
        lines.append(f"  faster: {winner}  (fa_gen / sdpa = {ratio:.2f}x); "
                     f"max |out difference| {diff:.3e}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    sys.exit(main())
