"""Document-masked (segment-id) attention off the GPU: the torch reference
path of ops.flash_attention against a dense masked softmax written here,
segment_ids_from_cu_seqlens, the argument rules, a packed Llama-tiny against
each document run alone, and ring attention with travelling kv ids."""
import math

import pytest
import torch
import torch.nn.functional as F

from vescale_amd.dtensor import DTensor, Shard

from tests.common import spawn


@pytest.fixture(autouse=True)
def _no_intra_op_pool():
    """As in test_flash_attention_general.py: the in-process math must not
    start the intra-op thread pool, the spawn tests fork this process."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _ids(*runs):
    """[(id, length), ...] -> ids of one row."""
    return torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in runs])


# ------------------------------------------------------------ reference path
def _dense(q, k, v, causal, shift, scale, q_seg, kv_seg):
    """softmax(masked scores) @ v in fp32, written out densely: (out, lse,
    live) with out = 0 and lse = -inf on rows that see no key."""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    kx = k.repeat_interleave(Hq // Hkv, 1)
    vx = v.repeat_interleave(Hq // Hkv, 1)
    vis = q_seg[:, :, None] == kv_seg[:, None, :]                  # [B, Sq, Sk]
    if causal:
        i = torch.arange(Sq)[:, None]
        j = torch.arange(Sk)[None, :]
        vis = vis & (j <= i + shift)
    live = vis.any(-1)                                             # [B, Sq]
    s = (q @ kx.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis[:, None], float("-inf"))
    # a dead row's scores are replaced before the softmax (no NaN in the
    # graph) and its results selected away after it
    s = s.masked_fill(~live[:, None, :, None], 0.0)
    lv = live[:, None, :, None].to(s.dtype)
    out = (torch.softmax(s, -1) * lv) @ vx
    lse = torch.where(live[:, None], torch.logsumexp(s, -1),
                      torch.full((), float("-inf")))
    return out, lse, live


# name: (Hq, Hkv, Sq, Sk, causal, shift, q ids [B, Sq], kv ids [B, Sk])
_REF_CASES = {
    "causal_docs": (4, 4, 33, 33, True, 0,
                    torch.stack([_ids((0, 5), (1, 20), (2, 8)), _ids((7, 33))]), None),
    "noncausal_gqa": (4, 2, 40, 40, False, 0,
                      torch.stack([_ids((3, 17), (1, 23)), _ids((0, 1), (5, 39))]), None),
    "unsorted": (4, 2, 31, 31, True, 0,
                 torch.stack([torch.arange(31) % 3, (torch.arange(31) * 7) % 4]), None),
    "unsorted_noncausal_mqa": (4, 1, 17, 29, False, 0,
                               torch.stack([torch.arange(17) % 3, torch.arange(17) % 2]),
                               torch.stack([torch.arange(29) % 3, (torch.arange(29) + 1) % 2])),
    "cross_shift": (4, 2, 20, 50, True, 30,
                    torch.stack([_ids((0, 8), (1, 12)), _ids((4, 20))]),
                    torch.stack([_ids((2, 30), (0, 8), (1, 12)), _ids((4, 50))])),
    # batch row 0: q id 9 is carried by no key (5 dead rows), kv id 6 by no
    # query (keys 20..29 get zero dk/dv); row 1 is ordinary
    "absent_ids": (4, 2, 24, 30, False, 0,
                   torch.stack([_ids((0, 10), (9, 5), (1, 9)), _ids((2, 24))]),
                   torch.stack([_ids((0, 10), (1, 10), (6, 10)), _ids((2, 30))])),
}


@pytest.mark.parametrize("name", sorted(_REF_CASES))
def test_reference_matches_dense_masked_softmax(name):
    from vescale_amd.ops import flash_attention

    Hq, Hkv, Sq, Sk, causal, shift, q_seg, kv_seg = _REF_CASES[name]
    B, D = 2, 16
    sc = 1.0 / math.sqrt(D)
    q, k, v = _rand((B, Hq, Sq, D), 1), _rand((B, Hkv, Sk, D), 2), _rand((B, Hkv, Sk, D), 3)
    wo, wl = _rand((B, Hq, Sq, D), 4), _rand((B, Hq, Sq), 5)

    q1, k1, v1 = (t.clone().requires_grad_(True) for t in (q, k, v))
    out, lse = flash_attention(q1, k1, v1, is_causal=causal, causal_shift=shift,
                               return_lse=True, q_segment_ids=q_seg,
                               kv_segment_ids=kv_seg)
    q2, k2, v2 = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref_o, ref_l, live = _dense(q2, k2, v2, causal, shift, sc, q_seg,
                                q_seg if kv_seg is None else kv_seg)
    dead = ~live[:, None].expand(B, Hq, Sq)

    assert lse.shape == (B, Hq, Sq) and lse.dtype == torch.float32
    assert (out[dead] == 0).all() and (lse[dead] == float("-inf")).all()
    assert torch.equal(lse == float("-inf"), dead)
    assert torch.allclose(out, ref_o, atol=1e-5)
    assert torch.allclose(lse[~dead], ref_l[~dead], atol=1e-5)

    def loss(o, l):
        return (o * wo).sum() + (torch.where(l > float("-inf"), l, 0.0) * wl).sum()

    loss(out, lse).backward()
    loss(ref_o, ref_l).backward()
    for got, want in ((q1, q2), (k1, k2), (v1, v2)):
        assert not torch.isnan(got.grad).any()
        assert torch.allclose(got.grad, want.grad, atol=1e-4)
    assert (q1.grad[dead] == 0).all()
    if name == "absent_ids":
        assert int(dead[0, 0].sum()) == 5 and not dead[1].any()
        assert (k1.grad[0, :, 20:] == 0).all() and (v1.grad[0, :, 20:] == 0).all()
        assert (k1.grad[0, :, :20] != 0).any()
    else:
        assert not dead.any()


def test_dead_rows_ignore_incoming_gradients():
    """A raw gradient into out and lse of rows whose id no key carries gives
    exactly zero input gradients there, and nothing is NaN."""
    from vescale_amd.ops import flash_attention

    q, k, v = (_rand((1, 2, 8, 16), s).requires_grad_(True) for s in (1, 2, 3))
    out, lse = flash_attention(q, k, v, return_lse=True,
                               q_segment_ids=torch.full((1, 8), 1),
                               kv_segment_ids=torch.full((1, 8), 2))
    assert (out == 0).all() and (lse == float("-inf")).all()
    for g in torch.autograd.grad([out, lse], [q, k, v],
                                 [torch.ones_like(out), torch.ones_like(lse)]):
        assert (g == 0).all()


# ------------------------------------------------------------ helper, argument rules
def test_segment_ids_from_cu_seqlens():
    from vescale_amd.ops import segment_ids_from_cu_seqlens

    ids = segment_ids_from_cu_seqlens([0, 5, 16], 16)
    assert ids.dtype == torch.int32 and ids.shape == (16,)
    assert ids.tolist() == [0] * 5 + [1] * 11
    # padding tail: an id of its own
    ids = segment_ids_from_cu_seqlens(torch.tensor([0, 3, 4, 9], dtype=torch.int32), 12)
    assert ids.dtype == torch.int32
    assert ids.tolist() == [0] * 3 + [1] + [2] * 5 + [3] * 3
    assert segment_ids_from_cu_seqlens([0], 3).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        segment_ids_from_cu_seqlens([0, 5, 17], 16)


def test_padding_attends_only_to_padding():
    from vescale_amd.ops import flash_attention, segment_ids_from_cu_seqlens

    ids = segment_ids_from_cu_seqlens([0, 4, 7], 10).unsqueeze(0)
    q, k, v = _rand((1, 2, 10, 16), 1), _rand((1, 2, 10, 16), 2), _rand((1, 2, 10, 16), 3)
    out = flash_attention(q, k, v, q_segment_ids=ids)
    pad = F.scaled_dot_product_attention(q[:, :, 7:], k[:, :, 7:], v[:, :, 7:])
    doc = F.scaled_dot_product_attention(q[:, :, 4:7], k[:, :, 4:7], v[:, :, 4:7])
    assert torch.allclose(out[:, :, 7:], pad, atol=1e-5)
    assert torch.allclose(out[:, :, 4:7], doc, atol=1e-5)


def test_argument_rules():
    from vescale_amd.ops import flash_attention

    q, k = _rand((1, 2, 4, 16), 0), _rand((1, 2, 6, 16), 1)
    qs, ks = torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, 6, dtype=torch.int64)
    # Sq != Sk: both are required
    with pytest.raises(ValueError):
        flash_attention(q, k, k, q_segment_ids=qs)
    with pytest.raises(ValueError):
        flash_attention(q, k, k, kv_segment_ids=ks)
    # kv ids alone are an error at Sq == Sk too
    with pytest.raises(ValueError):
        flash_attention(q, q, q, kv_segment_ids=qs)
    # shapes are [B, Sq] / [B, Sk]; ids are integers
    with pytest.raises(ValueError):
        flash_attention(q, k, k, q_segment_ids=qs, kv_segment_ids=qs)
    with pytest.raises(ValueError):
        flash_attention(q, k, k, q_segment_ids=ks, kv_segment_ids=ks)
    with pytest.raises(ValueError):
        flash_attention(q, q, q, q_segment_ids=qs.float())
    # q ids alone at Sq == Sk stand for both; any integer dtype; all ids
    # equal is no mask at all
    want = flash_attention(q, q, q, is_causal=True)
    for dt in (torch.int64, torch.int32, torch.int16, torch.uint8):
        got = flash_attention(q, q, q, is_causal=True, q_segment_ids=qs.to(dt) + 3)
        assert torch.equal(got, want)
    got = flash_attention(q, k, k, q_segment_ids=qs, kv_segment_ids=ks)
    assert torch.equal(got, flash_attention(q, k, k))


# ------------------------------------------------------------ Llama-tiny, packed vs alone
def test_llama_packed_equals_documents_alone():
    """Two documents of 5 and 11 tokens packed into one row of 16 with
    segment_ids: logits and parameter gradients of the summed loss are those
    of the two documents run alone (fp32, CPU)."""
    from vescale_amd.models.llama import LlamaModel, llama_tiny
    from vescale_amd.ops import segment_ids_from_cu_seqlens

    torch.manual_seed(0)
    cfg = llama_tiny(vocab=96, seq=16)
    model = LlamaModel(cfg)
    model.init_weights(std=0.1)
    g = torch.Generator().manual_seed(1)
    tokens = torch.randint(0, cfg.vocab_size, (1, 16), generator=g)
    targets = torch.roll(tokens, -1, dims=1)
    targets[0, 4] = targets[0, 15] = -100   # the last target of each document
    seg = segment_ids_from_cu_seqlens([0, 5, 16], 16).unsqueeze(0)

    def summed_loss(logits, tgt):
        return F.cross_entropy(logits.reshape(-1, cfg.vocab_size), tgt.reshape(-1),
                               ignore_index=-100, reduction="sum")

    def grads():
        out = {n: p.grad.clone() for n, p in model.named_parameters()}
        model.zero_grad()
        return out

    packed = model(tokens, segment_ids=seg)
    summed_loss(packed, targets).backward()
    g_packed = grads()

    alone = [model(tokens[:, a:b]) for a, b in ((0, 5), (5, 16))]
    (summed_loss(alone[0], targets[:, :5]) + summed_loss(alone[1], targets[:, 5:])).backward()
    g_alone = grads()

    assert torch.allclose(packed[:, :5], alone[0], atol=1e-5)
    assert torch.allclose(packed[:, 5:], alone[1], atol=1e-5)
    assert set(g_packed) == set(g_alone) and g_packed
    for n in g_packed:
        assert torch.allclose(g_packed[n], g_alone[n], atol=1e-4), n
    # and the mask is what does it: without ids document 2 reads document 1
    unmasked = model(tokens)
    assert not torch.allclose(unmasked[:, 5:], alone[1], atol=1e-3)


def test_mixtral_block_threads_segment_ids():
    from vescale_amd.models.mixtral import MixtralBlock, MixtralConfig
    from vescale_amd.ops import build_rope_table

    torch.manual_seed(0)
    cfg = MixtralConfig(dim=32, n_layers=1, n_heads=2, n_kv_heads=1, ffn_dim=64,
                        vocab_size=64, max_seq_len=16, n_experts=2, top_k=1)
    blk = MixtralBlock(cfg)
    tab = build_rope_table(cfg.max_seq_len, cfg.head_dim, cfg.rope_theta)
    x = _rand((1, 16, 32), 2)
    seg = torch.cat([torch.zeros(5), torch.ones(11)]).long().unsqueeze(0)
    a = blk.attn(blk.attn_norm(x), tab, seg)
    alone = blk.attn(blk.attn_norm(x[:, :5]), tab)
    assert torch.allclose(a[:, :5], alone, atol=1e-5)
    assert blk(x, tab, seg).shape == x.shape


# ------------------------------------------------------------ ring, impl="flash"
def _grad_full(t):
    return t.grad.full_tensor() if isinstance(t.grad, DTensor) else t.grad


def _t_ring_flash_segments(rank, ws, B, Hq, Hkv, S, D, seed):
    """ring_sdpa(impl="flash", segment_ids=local slice): output and all three
    grads match the single-process segment-masked attention; the kv ids
    travel the ring as one extra plain tensor per hop."""
    import vescale_amd.dmodule.ring_attention as ra
    from vescale_amd.dtensor import distribute_tensor, init_device_mesh
    from vescale_amd.ops import flash_attention

    mesh = init_device_mesh("cpu", (ws,))
    g = torch.Generator().manual_seed(seed)
    qg = torch.randn(B, Hq, S, D, generator=g, requires_grad=True)
    kg = torch.randn(B, Hkv, S, D, generator=g, requires_grad=True)
    vg = torch.randn(B, Hkv, S, D, generator=g, requires_grad=True)
    # row 0: three documents, the second across the rank boundary, the third
    # wholly on the last rank (its rows are dead in every earlier block);
    # row 1: unsorted ids
    seg = torch.stack([_ids((0, 3), (1, S // 2), (2, S - 3 - S // 2)),
                       torch.arange(S) % 3][:B])
    sl = S // ws
    seg_local = seg[:, rank * sl:(rank + 1) * sl]

    shifted = []
    orig_shift = ra._shift

    def recording_shift(t, group, *, forward):
        if forward:
            shifted.append((tuple(t.shape), t.dtype))
        return orig_shift(t, group, forward=forward)

    ra._shift = recording_shift
    try:
        for causal in (False, True):
            q = distribute_tensor(qg.detach().clone().requires_grad_(True), mesh, [Shard(2)])
            k = distribute_tensor(kg.detach().clone().requires_grad_(True), mesh, [Shard(2)])
            v = distribute_tensor(vg.detach().clone().requires_grad_(True), mesh, [Shard(2)])
            out = ra.ring_sdpa(q, k, v, is_causal=causal, impl="flash",
                               segment_ids=seg_local)
            assert out.placements[0].is_shard(2)
            ref = flash_attention(qg, kg, vg, is_causal=causal, q_segment_ids=seg)
            full = out.full_tensor()
            assert not torch.isnan(full).any()
            assert torch.allclose(full, ref, atol=1e-5), causal
            # not the unmasked result
            plain = flash_attention(qg, kg, vg, is_causal=causal)
            assert not torch.allclose(full, plain, atol=1e-3)

            out.to_local().pow(2).sum().backward()
            ref.pow(2).sum().backward()
            for dt, pl in ((q, qg), (k, kg), (v, vg)):
                gd = _grad_full(dt)
                assert not torch.isnan(gd).any()
                assert torch.allclose(gd, pl.grad, atol=1e-5), causal
            qg.grad = kg.grad = vg.grad = None
    finally:
        ra._shift = orig_shift
    # per run and hop: k, v (Hkv heads) and the int32 kv ids
    assert len(shifted) == 2 * 3 * (ws - 1), shifted
    ids = [s for s in shifted if s[1] == torch.int32]
    assert len(ids) == 2 * (ws - 1) and all(s[0] == (B, sl) for s in ids), shifted

    with pytest.raises(ValueError):
        ra.ring_sdpa(q, k, v, is_causal=True, impl="eager", segment_ids=seg_local)
    with pytest.raises(ValueError):
        ra.ring_sdpa(q, k, v, is_causal=True, segment_ids=seg_local)


@pytest.mark.parametrize("ws,B,Hq,Hkv,S,D,seed", [
    (2, 2, 4, 2, 16, 16, 4),     # GQA
    (4, 1, 2, 2, 16, 8, 5),      # multi-hop ring
])
def test_ring_flash_segments(ws, B, Hq, Hkv, S, D, seed):
    spawn(ws, _t_ring_flash_segments, B, Hq, Hkv, S, D, seed)
