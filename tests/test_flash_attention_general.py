"""ops.flash_attention off-GPU (the torch reference path: also the oracle of
the HIP kernel) and the opt-in impl="flash" of ring / Ulysses attention."""
import math

import pytest
import torch
import torch.nn.functional as F

from vescale_amd.dtensor import DTensor, Shard

from tests.common import spawn


@pytest.fixture(autouse=True)
def _no_intra_op_pool():
    """The in-process math here must not start the intra-op thread pool:
    the spawn tests of this and of later files fork this process, and a
    forked child of a process with a live OpenMP pool hangs in its first
    parallel region."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------ reference path
@pytest.mark.parametrize("Hq,Hkv,Sq,Sk,causal", [
    (4, 4, 33, 33, True),     # square causal
    (4, 4, 33, 33, False),    # non-causal
    (4, 2, 40, 40, True),     # GQA
    (4, 1, 17, 29, False),    # MQA, rectangular
    (4, 2, 20, 50, True),     # Sq != Sk, shift 0 = SDPA's top-left alignment
    (4, 2, 50, 20, True),
])
def test_reference_path_matches_sdpa(Hq, Hkv, Sq, Sk, causal):
    from vescale_amd.ops import flash_attention

    q, k, v = _rand((2, Hq, Sq, 16), 1), _rand((2, Hkv, Sk, 16), 2), _rand((2, Hkv, Sk, 16), 3)
    out = flash_attention(q, k, v, is_causal=causal)
    ref = F.scaled_dot_product_attention(q, k, v, is_causal=causal, enable_gqa=Hq != Hkv)
    assert out.dtype == q.dtype
    assert torch.allclose(out, ref, atol=1e-5)
    out2 = flash_attention(q, k, v, is_causal=causal, scale=0.3)
    ref2 = F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=0.3,
                                          enable_gqa=Hq != Hkv)
    assert torch.allclose(out2, ref2, atol=1e-5)


def test_shift_needs_causal():
    from vescale_amd.ops import flash_attention

    q = _rand((1, 1, 4, 16), 0)
    with pytest.raises(ValueError):
        flash_attention(q, q, q, causal_shift=1)


def _fp64_oracle(q, k, v, shift, scale):
    """Plain fp64 attention, live rows only (dead rows are asserted apart)."""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    kx = k.repeat_interleave(Hq // Hkv, 1)
    vx = v.repeat_interleave(Hq // Hkv, 1)
    s = (q @ kx.transpose(-1, -2)) * scale
    i = torch.arange(Sq).unsqueeze(1)
    j = torch.arange(Sk).unsqueeze(0)
    live = torch.arange(Sq) + shift >= 0
    s = s[:, :, live].masked_fill((j > i + shift)[live], float("-inf"))
    return torch.softmax(s, -1) @ vx, torch.logsumexp(s, -1), live


@pytest.mark.parametrize("shift", [130, 0, -5, -70])   # Sk-Sq, 0, -5, -Sq
def test_lse_and_gradients_vs_fp64(shift):
    from vescale_amd.ops import flash_attention

    B, Hq, Hkv, Sq, Sk, D = 2, 4, 2, 70, 200, 64
    sc = 1.0 / math.sqrt(D)
    q, k, v = _rand((B, Hq, Sq, D), 4), _rand((B, Hkv, Sk, D), 5), _rand((B, Hkv, Sk, D), 6)
    wo, wl = _rand((B, Hq, Sq, D), 7), _rand((B, Hq, Sq), 8)

    q1, k1, v1 = (t.clone().requires_grad_(True) for t in (q, k, v))
    out, lse = flash_attention(q1, k1, v1, is_causal=True, causal_shift=shift,
                               return_lse=True)
    assert lse.shape == (B, Hq, Sq) and lse.dtype == torch.float32

    q2, k2, v2 = (t.double().requires_grad_(True) for t in (q, k, v))
    ref_o, ref_l, live = _fp64_oracle(q2, k2, v2, shift, sc)
    dead = ~live
    assert int(dead.sum()) == {130: 0, 0: 0, -5: 5, -70: 70}[shift]

    # dead rows: exact
    assert (out[:, :, dead] == 0).all()
    assert (lse[:, :, dead] == float("-inf")).all()
    # live rows: lse is the masked logsumexp
    assert torch.allclose(lse[:, :, live].double(), ref_l, atol=1e-5)
    assert torch.allclose(out[:, :, live].double(), ref_o, atol=1e-5)

    # a loss that uses both outputs (and, on dead rows, only values that
    # must not matter: out = 0 and a where()-discarded -inf)
    loss = (out * wo).sum() + (torch.where(lse > float("-inf"), lse, 0.0) * wl).sum() \
        + (out[:, :, dead] * 3.0).sum()
    loss.backward()
    if live.any():
        ref_loss = (ref_o * wo[:, :, live].double()).sum() + (ref_l * wl[:, :, live].double()).sum()
        ref_loss.backward()
    for got, want in ((q1, q2), (k1, k2), (v1, v2)):
        assert not torch.isnan(got.grad).any()
        w = want.grad if want.grad is not None else torch.zeros_like(want)
        assert torch.allclose(got.grad.double(), w, atol=1e-5)
    assert (q1.grad[:, :, dead] == 0).all()
    if bool(dead.all()):
        assert (k1.grad == 0).all() and (v1.grad == 0).all()


def test_dead_rows_ignore_incoming_lse_gradient():
    """dlse is taken as 0 on dead rows: a raw gradient into lse = -inf rows
    yields exactly zero input gradients, and nothing is NaN."""
    from vescale_amd.ops import flash_attention

    q, k, v = (_rand((1, 2, 8, 16), s).requires_grad_(True) for s in (1, 2, 3))
    out, lse = flash_attention(q, k, v, is_causal=True, causal_shift=-8, return_lse=True)
    assert (out == 0).all() and (lse == float("-inf")).all()
    gq, gk, gv = torch.autograd.grad([out, lse], [q, k, v],
                                     [torch.ones_like(out), torch.ones_like(lse)])
    for g in (gq, gk, gv):
        assert (g == 0).all()


# ------------------------------------------------------------ ring, impl="flash"
def _grad_full(t):
    return t.grad.full_tensor() if isinstance(t.grad, DTensor) else t.grad


def _t_ring_flash(rank, ws, B, Hq, Hkv, S, D, seed):
    """impl="flash" ring attention: output and all three grads match
    single-device SDPA; k/v travel the ring with Hkv heads."""
    import vescale_amd.dmodule.ring_attention as ra
    from vescale_amd.dtensor import distribute_tensor, init_device_mesh

    mesh = init_device_mesh("cpu", (ws,))
    g = torch.Generator().manual_seed(seed)
    qg = torch.randn(B, Hq, S, D, generator=g, requires_grad=True)
    kg = torch.randn(B, Hkv, S, D, generator=g, requires_grad=True)
    vg = torch.randn(B, Hkv, S, D, generator=g, requires_grad=True)

    shifted = []
    orig_shift = ra._shift

    def recording_shift(t, group, *, forward):
        if forward:
            shifted.append(tuple(t.shape))
        return orig_shift(t, group, forward=forward)

    ra._shift = recording_shift
    try:
        for causal in (False, True):
            q = distribute_tensor(qg.detach().clone().requires_grad_(True), mesh, [Shard(2)])
            k = distribute_tensor(kg.detach().clone().requires_grad_(True), mesh, [Shard(2)])
            v = distribute_tensor(vg.detach().clone().requires_grad_(True), mesh, [Shard(2)])
            attn = ra.RingAttention(is_causal=causal, impl="flash")
            out = attn(q, k, v)
            assert out.placements[0].is_shard(2)
            ref = F.scaled_dot_product_attention(qg, kg, vg, is_causal=causal,
                                                 enable_gqa=Hq != Hkv)
            full = out.full_tensor()
            assert not torch.isnan(full).any()
            assert torch.allclose(full, ref, atol=1e-5), causal

            out.to_local().pow(2).sum().backward()
            ref.pow(2).sum().backward()
            for dt, pl in ((q, qg), (k, kg), (v, vg)):
                gd = _grad_full(dt)
                assert not torch.isnan(gd).any()
                assert torch.allclose(gd, pl.grad, atol=1e-5), causal
            qg.grad = kg.grad = vg.grad = None
    finally:
        ra._shift = orig_shift
    # 2 tensors x (ws - 1) shifts x 2 runs, every one with Hkv heads
    assert len(shifted) == 4 * (ws - 1), shifted
    assert all(s == (B, Hkv, S // ws, D) for s in shifted), shifted


@pytest.mark.parametrize("ws,B,Hq,Hkv,S,D,seed", [
    (2, 2, 4, 4, 8, 16, 4),     # shapes of _t_ring_sdpa
    (2, 2, 4, 2, 8, 16, 4),     # its GQA case
    (4, 1, 2, 2, 16, 8, 5),     # shapes of _t_ring_sdpa_ws4
    (4, 1, 4, 2, 16, 8, 5),     # GQA on the multi-hop ring
])
def test_ring_flash(ws, B, Hq, Hkv, S, D, seed):
    spawn(ws, _t_ring_flash, B, Hq, Hkv, S, D, seed)


def _t_ring_default_is_eager(rank, ws):
    """The default path still expands GQA heads before circulating."""
    import vescale_amd.dmodule.ring_attention as ra
    from vescale_amd.dtensor import distribute_tensor, init_device_mesh

    mesh = init_device_mesh("cpu", (ws,))
    q = distribute_tensor(_rand((1, 4, 8, 8), 1), mesh, [Shard(2)])
    k = distribute_tensor(_rand((1, 2, 8, 8), 2), mesh, [Shard(2)])
    v = distribute_tensor(_rand((1, 2, 8, 8), 3), mesh, [Shard(2)])
    a = ra.ring_sdpa(q, k, v, is_causal=True)
    b = ra.ring_sdpa(q, k, v, is_causal=True, impl="eager")
    c = ra.ring_sdpa(q, k, v, is_causal=True, impl="flash")
    assert torch.equal(a.to_local(), b.to_local())
    assert torch.allclose(a.to_local(), c.to_local(), atol=1e-5)


def test_ring_default_is_eager():
    spawn(2, _t_ring_default_is_eager)


# ------------------------------------------------------------ Ulysses, impl="flash"
def _t_ulysses_flash(rank, ws):
    from vescale_amd.debug import CommDebugMode
    from vescale_amd.dmodule.ulysses import UlyssesAttention
    from vescale_amd.dtensor import distribute_tensor, init_device_mesh

    mesh = init_device_mesh("cpu", (ws,))
    B, H, S, D = 2, 4, 8, 16
    g = torch.Generator().manual_seed(3)
    qg = torch.randn(B, H, S, D, generator=g, requires_grad=True)
    kg = torch.randn(B, H, S, D, generator=g, requires_grad=True)
    vg = torch.randn(B, H, S, D, generator=g, requires_grad=True)
    for causal in (False, True):
        q = distribute_tensor(qg.detach().clone().requires_grad_(True), mesh, [Shard(2)])
        k = distribute_tensor(kg.detach().clone().requires_grad_(True), mesh, [Shard(2)])
        v = distribute_tensor(vg.detach().clone().requires_grad_(True), mesh, [Shard(2)])
        attn = UlyssesAttention(is_causal=causal, impl="flash")
        with CommDebugMode() as cm:
            out = attn(q, k, v)
        assert cm.get_comm_counts().get("mesh_all_to_all", 0) == 4, cm.get_comm_counts()
        assert out.placements[0].is_shard(2)
        ref = F.scaled_dot_product_attention(qg, kg, vg, is_causal=causal)
        assert torch.allclose(out.full_tensor(), ref, atol=1e-5)
        out.to_local().pow(2).sum().backward()
        ref.pow(2).sum().backward()
        for dt, pl in ((q, qg), (k, kg), (v, vg)):
            assert torch.allclose(_grad_full(dt), pl.grad, atol=1e-5), causal
        qg.grad = kg.grad = vg.grad = None


def test_ulysses_flash():
    spawn(2, _t_ulysses_flash)
