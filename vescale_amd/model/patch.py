"""Vocab-parallel module patches.

Parity: legacy/vescale/model/patch/vp_embedding.py:38 (range mask +
partial + allreduce) and vp_cross_entropy.py:43-149 (local max ->
allreduce-max -> masked gather -> allreduce-sum log-sum-exp; here the fused
ops.vocab_parallel_cross_entropy: two all-reduces, HIP kernels), as opt-in
module-level rewrites for models whose embedding/classifier weights are
vocab-sharded Shard(0).
"""
from __future__ import annotations


import torch
import torch.distributed as dist
import torch.nn as nn

from ..dtensor import DeviceMesh, DTensor, Partial, Replicate, Shard
from ..dtensor import _collective_utils as cc
from ..dtensor.placement_types import TensorMeta
from ..dtensor._dtensor_spec import DTensorSpec


class VocabParallelEmbedding(nn.Module):
    """Embedding with Shard(0) (vocab-sharded) weight; output allreduced.

    Accepts a plain nn.Embedding to wrap; the weight may already be a
    DTensor (from parallelize_module) or a plain tensor to distribute.
    """

    def __init__(self, emb: nn.Embedding, mesh: DeviceMesh, mesh_dim: int = 0):
        super().__init__()
        self.mesh = mesh
        self.mesh_dim = mesh_dim
        self.num_embeddings = emb.num_embeddings
        w = emb.weight
        if not isinstance(w.data, DTensor):
            from ..dtensor import distribute_tensor

            d = distribute_tensor(w.data, mesh, [Shard(0)] + [Replicate()] * (mesh.ndim - 1))
            self.weight = nn.Parameter(d, requires_grad=w.requires_grad)
        else:
            self.weight = w

    def forward(self, idx: torch.Tensor) -> torch.Tensor:
        import torch.nn.functional as F

        if not isinstance(idx, DTensor):
            idx = DTensor.from_local(idx, self.mesh, [Replicate()] * self.mesh.ndim)
        out = F.embedding(idx, self.weight)  # vocab-parallel handler -> Partial
        if isinstance(out, DTensor) and any(p.is_partial() for p in out.placements):
            out = out.redistribute(placements=[
                Replicate() if p.is_partial() else p for p in out.placements
            ])
        return out


def _vocab_parallel_ce(logits_local, target, start, vocab_total, mesh, mesh_dim):
    """Per-token loss over a [..., V/w] raw logits shard: the fused
    vocab-parallel CE of ops (two all-reduces over the mesh dim, none in
    backward; HIP kernels when the shard is bf16 on the GPU)."""
    from ..ops import vocab_parallel_cross_entropy

    group = mesh.get_group(mesh_dim) if mesh.size(mesh_dim) > 1 else None
    n = logits_local.shape[-1]
    loss = vocab_parallel_cross_entropy(
        logits_local.reshape(-1, n), target.reshape(-1), start, vocab_total,
        group=group, ignore_index=-100, reduction="none")
    return loss.reshape(target.shape)


class VocabParallelCrossEntropy(nn.Module):
    """CE over vocab-sharded raw logits — per-token loss vector output
    (reduction applied by caller), numerically matching dense CE."""

    def __init__(self, mesh: DeviceMesh, mesh_dim: int = 0):
        super().__init__()
        self.mesh = mesh
        self.mesh_dim = mesh_dim

    def forward(self, logits, target):
        if isinstance(logits, DTensor):
            spec = logits._spec
            vocab = spec.shape[-1]
            md = None
            for i, p in enumerate(spec.placements):
                if isinstance(p, Shard) and p.dim == spec.ndim - 1:
                    md = i
            assert md is not None, "logits must be vocab-sharded"
            w = self.mesh.size(md)
            r = self.mesh.get_local_rank(md)
            start = Shard.chunk_offset(vocab, w, r)
            local = logits._local_tensor
            tgt = target.to_local() if isinstance(target, DTensor) else target
            loss = _vocab_parallel_ce(local, tgt, start, vocab, self.mesh, md)
            return loss
        # dense fallback
        import torch.nn.functional as F

        return F.cross_entropy(logits, target, reduction="none")
