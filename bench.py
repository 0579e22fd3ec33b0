"""Flagship benchmark — Llama-3-8B veScale-FSDP-style training step on
MI355X (BASELINE.json metric: tokens/sec whole node at 1/2/4/8 GPUs).

Driver contract:
  python bench.py --gpus N --steps K --warmup W
  (N>1 launched via torch.distributed.run, one rank per GPU over RCCL)

Synthetic data (random tokens), random-init weights, bf16 compute, weak
scaling (per-GPU batch fixed).  Times exactly K steps bracketed by
barrier + torch.cuda.synchronize on both sides; MAX over ranks; rank 0
prints ONE JSON line.

A plain run does only what the headline figure needs: set up, warm up,
time the K steps, print.  Options:
  --dump-outputs DIR  after the timed steps, rank 0 writes what the timed
                      step left behind in its LAST step as DIR/<name>.npy
                      (float32): `loss` — the value step() returns — and
                      `params_sample` — a fixed, seeded sample of the
                      updated parameter shards.  Inputs, init and sample
                      indices are seeded, so two builds run with the same
                      arguments can be compared array for array.  The
                      train step uses no atomic accumulation, so two runs
                      of one build write bitwise-equal files (checked at
                      8B on MI355X, graph-replayed path).  With more than
                      one rank only rank 0 writes: its local loss and a
                      sample of its own shards.  If hipGraph capture falls
                      back to the eager path the dumped loss is the last
                      eager step's (repeatability not checked there).
  --full              extended measurements that need runs of their own
                      (secondary configs, baselines, per-kernel figures) go
                      behind this flag.  The benchmark has none today — the
                      flag is accepted so callers can rely on it.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch
import torch.distributed as dist


_DUMP_SAMPLE_PER_UNIT = 65536  # x ~33 units x 4 B: ~9 MB for Llama-3-8B


def dump_outputs(out_dir, loss, eng):
    """Write the last timed step's results as float32 .npy files: the loss
    step() returned and a seeded sample of every unit's updated flat
    parameter shard (the full 8B shard set would be ~32 GB)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"),
            loss.detach().float().reshape(1).cpu().numpy())
    pieces = []
    for i, u in enumerate(eng.units):
        gen = torch.Generator(device="cpu").manual_seed(9176 + i)
        k = min(_DUMP_SAMPLE_PER_UNIT, u.shard_numel)
        idx = torch.randint(0, u.shard_numel, (k,), generator=gen)
        pieces.append(u.shard.detach()[idx.to(u.shard.device)].float().cpu())
    np.save(os.path.join(out_dir, "params_sample.npy"),
            torch.cat(pieces).numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", type=str, default="llama3_8b",
                    choices=["llama3_8b", "llama3_70b", "llama_tiny"])
    ap.add_argument("--batch", type=int, default=4, help="per-GPU batch size")
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--activation-checkpointing", action="store_true")
    ap.add_argument("--no-master-weights", action="store_true")
    ap.add_argument("--tp", type=int, default=1,
                    help="tensor-parallel degree (BASELINE 2D config: TP x FSDP)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs to DIR/<name>.npy "
                         "(rank 0 only: its local loss and its own shards)")
    ap.add_argument("--full", action="store_true",
                    help="also run the extended measurements (none today)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = max(world_size, 1)

    on_gpu = torch.cuda.is_available()
    ndev = torch.cuda.device_count() if on_gpu else 0
    device = torch.device(f"cuda:{local_rank % max(ndev, 1)}") if on_gpu else torch.device("cpu")
    if on_gpu:
        torch.cuda.set_device(device)

    if world_size > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("VESCALE_BENCH_BACKEND", "nccl" if on_gpu else "gloo")
        dist.init_process_group(backend)

    from vescale_amd.dtensor import init_device_mesh
    from vescale_amd.fsdp import FSDP, FlatAdamW
    from vescale_amd.models import llama as M

    cfg = getattr(M, args.model)() if args.model != "llama_tiny" else M.llama_tiny()
    if not on_gpu and args.model != "llama_tiny":
        # CPU smoke: shrink so the default invocation finishes in minutes
        cfg = M.llama_tiny()
        args.batch, args.seq = 2, 64

    torch.manual_seed(1234)
    tp = args.tp
    assert world_size % tp == 0, "world size must be divisible by --tp"
    dp = world_size // tp
    tp_group = None
    if world_size > 1:
        if tp > 1:
            mesh = init_device_mesh(device.type, (dp, tp), mesh_dim_names=("DP", "TP"))
            tp_group = mesh.get_group(1)
        else:
            mesh = init_device_mesh(device.type, (world_size,), mesh_dim_names=("DP",))
    else:
        mesh = None

    with torch.device("meta"):
        model = M.LlamaModel(cfg, tp_group=tp_group)
    model = model.to_empty(device=device)
    model.rope_table.copy_(
        M.build_rope_table(cfg.max_seq_len, cfg.head_dim, cfg.rope_theta).to(device)
    )
    model.init_weights()
    model.activation_checkpointing = args.activation_checkpointing
    dtype = torch.bfloat16 if on_gpu else torch.float32

    if world_size > 1:
        eng = FSDP(model, mesh, mesh_dim=0, param_dtype=dtype, device=device)
    else:
        eng = FSDP(model, None, param_dtype=dtype, device=device)
    opt = FlatAdamW(eng, lr=args.lr, grad_clip=1.0,
                    use_master_weights=not args.no_master_weights)

    B, S = args.batch, args.seq
    dp_rank = rank // tp  # TP ranks share the batch
    gen = torch.Generator(device="cpu").manual_seed(4321 + dp_rank)
    x = torch.randint(0, cfg.vocab_size, (B, S), generator=gen).to(device)
    y = torch.roll(x, -1, dims=1)

    def step():
        loss = eng(x, y)
        loss.backward()
        opt.step()
        return loss

    for _ in range(args.warmup):
        step()

    # hipGraph the whole train step (fwd+bwd+fused AdamW): the single-GPU
    # step is ~10% host-launch-bound (round-1 rocprof: GPU busy 90%);
    # capturing removes per-launch dispatch cost.  Single-rank only for
    # now — the multi-rank path keeps eager RCCL collectives.  Disable
    # with VESCALE_GRAPH=0.  Requirements satisfied by construction:
    # static input (synthetic fixed batch), no dropout, no host syncs in
    # FlatAdamW (device-side clip scale).
    graph = None
    static_loss = None
    if (
        on_gpu
        and world_size == 1
        and os.environ.get("VESCALE_GRAPH", "1") not in ("0", "false")
    ):
        try:
            # one more eager step before capture, on the CURRENT stream: a
            # fresh side stream cannot reuse the warmup's cached blocks and
            # re-allocates the whole activation set (~5 s of hipMalloc at
            # 8B), while capture runs on torch.cuda.graph's own stream and
            # private pool either way
            step()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                static_loss = step()
            g.replay()  # one untimed replay to validate
            torch.cuda.synchronize()
            graph = g
        except Exception as e:  # fall back to eager, report why
            import sys

            print(f"[bench] hipGraph capture failed ({e}); eager path",
                  file=sys.stderr)
            graph = None

    if graph is not None:
        def step():  # noqa: F811 — replay the captured step
            graph.replay()
            return static_loss

    if world_size > 1:
        dist.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    if on_gpu:
        torch.cuda.synchronize()
    if world_size > 1:
        dist.barrier()
    t1 = time.perf_counter()

    # MAX over ranks (nccl backend: reduce on-device — a CPU tensor would
    # raise under RCCL)
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=device)
    if world_size > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    sec = float(elapsed.item())
    ms_per_step = sec / args.steps * 1e3
    tokens_per_step = B * S * (n_gpus // tp)
    tok_s = tokens_per_step * args.steps / sec

    # MFU per the reference's estimator (open_llama_4D_benchmark/
    # llama_mfu_calculator.py:22-29 — 3x forward FLOPs, Kaplan-style) with
    # the MI355X bf16 DENSE peak (2.5 PF/GPU; AMD's 5 PF figure is 2:1-
    # sparse) in place of the A100/H100 table.
    n_params = cfg.num_params()
    emb = cfg.vocab_size * cfg.dim
    fwd_flops_per_tok = 2 * (n_params - emb) + (
        2 * 2 * cfg.n_layers * cfg.dim * S * 0.5  # causal attention
    )
    total_flops = 3 * fwd_flops_per_tok * tokens_per_step
    mfu = total_flops / sec * args.steps / (n_gpus * 2.5e15)

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loss, eng)

    if rank == 0:
        out = {
            "metric": "tokens/sec (whole node) Llama-3-8B veScale-FSDP",
            "value": tok_s,
            "unit": "tokens/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if on_gpu else "fp32-cpu-smoke",
            "data": "synthetic",
            "config": {
                "model": args.model if on_gpu else "llama_tiny(cpu-smoke)",
                "global_batch": B * dp,
                "seq_len": S,
                "parallelism": f"tp{tp}_fsdp{dp}" if tp > 1 else f"fsdp{n_gpus}",
                "final_loss": float(loss.detach().float().cpu()),
                "mfu_est": round(mfu, 4),
                "mfu_peak_ref": "2.5 PF bf16 dense per MI355X",
                "activation_checkpointing": args.activation_checkpointing,
                "hipgraph": graph is not None,
            },
        }
        print(json.dumps(out))

    if world_size > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
