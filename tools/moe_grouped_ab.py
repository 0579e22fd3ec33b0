"""A/B of the MoE expert FFN backends (VESCALE_MOE_GEMM=loop|grouped) on one
Mixtral-8x7B MoE layer, forward + backward: dim 4096, ffn 14336, 8 experts,
top-2, 8192 tokens, bf16.

    python tools/moe_grouped_ab.py [--reps 10] [--out profiles/moe_grouped_ab.txt]

The two backends alternate inside one process and one call, per routing:
  random  - top-2 of random router logits
  skewed  - every token's first choice is expert 0 (half of all rows), the
            second uniform over the others
Each sample is one forward + backward between device events; reported are
the median and the spread (max - min) of each backend, and the difference of
the outputs of the two on the same inputs.  `grouped` earns the default only
if it is faster at BOTH routings by more than the larger of the two spreads.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vescale_amd.models.mixtral import MoELayer, mixtral_8x7b  # noqa: E402

BACKENDS = ("loop", "grouped")


def routing(kind, tokens, n_experts, device):
    g = torch.Generator(device="cpu").manual_seed(1)
    if kind == "random":
        ids = torch.topk(torch.randn(tokens, n_experts, generator=g), 2, dim=-1)[1]
    else:
        second = torch.randint(1, n_experts, (tokens, 1), generator=g)
        ids = torch.cat([torch.zeros(tokens, 1, dtype=torch.int64), second], dim=1)
    weights = torch.softmax(torch.randn(tokens, 2, generator=g), dim=-1)
    return weights.to(device, torch.bfloat16), ids.to(device)


def step(layer, x, weights, ids, dout, backend):
    os.environ["VESCALE_MOE_GEMM"] = backend
    layer.zero_grad(set_to_none=True)
    x.grad = None
    out = layer._dense_moe(x, weights, ids)
    out.backward(dout)
    return out


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda")
    cfg = mixtral_8x7b()
    torch.manual_seed(0)
    with dev:  # 1.4e9 parameters: built and initialised on the device
        layer = MoELayer(cfg).to(torch.bfloat16)
    for p in layer.parameters():
        torch.nn.init.normal_(p, std=0.02)
    x = torch.randn(args.tokens, cfg.dim, device=dev).to(torch.bfloat16).requires_grad_()
    dout = torch.randn(args.tokens, cfg.dim, device=dev).to(torch.bfloat16)
    rows = args.tokens * cfg.top_k
    flop = 3 * 2 * rows * 3 * cfg.ffn_dim * cfg.dim  # fwd + dgrad + wgrad of w13 and w2
    lines = [f"MoE layer fwd+bwd, dim {cfg.dim} ffn {cfg.ffn_dim} E {cfg.n_experts} top-{cfg.top_k} "
             f"tokens {args.tokens} bf16, {args.reps} alternating samples, {flop / 1e12:.2f} TFLOP"]
    verdict = []
    for kind in ("random", "skewed"):
        weights, ids = routing(kind, args.tokens, cfg.n_experts, dev)
        counts = torch.bincount(ids.reshape(-1), minlength=cfg.n_experts).tolist()
        outs = {b: step(layer, x, weights, ids, dout, b).detach().float() for b in BACKENDS}
        diff = float((outs["loop"] - outs["grouped"]).abs().max())
        scale = float(outs["loop"].abs().max())
        del outs
        for _ in range(args.warmup):
            for b in BACKENDS:
                step(layer, x, weights, ids, dout, b)
        ms = {b: [] for b in BACKENDS}
        for _ in range(args.reps):
            for b in BACKENDS:
                ms[b].append(timed(lambda: step(layer, x, weights, ids, dout, b)))
        lines.append(f"routing {kind}: rows per expert {counts}; "
                     f"max |out_loop - out_grouped| {diff:.3e} (max |out| {scale:.3e})")
        med = {b: statistics.median(ms[b]) for b in BACKENDS}
        spread = {b: max(ms[b]) - min(ms[b]) for b in BACKENDS}
        for b in BACKENDS:
            lines.append(f"  {b:8s} median {med[b]:8.3f} ms  spread {spread[b]:7.3f} ms  "
                         f"min {min(ms[b]):8.3f}  max {max(ms[b]):8.3f}  "
                         f"{flop / med[b] / 1e9:7.1f} TFLOP/s")
        verdict.append(med["loop"] - med["grouped"] > max(spread.values()))
    lines.append("grouped faster than loop by more than the larger spread at both routings: "
                 + ("yes" if all(verdict) else "no"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
