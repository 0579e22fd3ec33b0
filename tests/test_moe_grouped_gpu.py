"""MoELayer with VESCALE_MOE_GEMM=grouped against the per-expert loop and an fp32
CPU run with the bf16 run's routing ids: grouped error <= 2 x loop error + one
bf16 ulp of the reference's max.  The grouped forward has no host sync."""
import math

import pytest
import torch

from vescale_amd.models.mixtral import MixtralConfig, MoELayer

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")]


def _layer_and_input():
    torch.manual_seed(0)
    cfg = MixtralConfig(dim=128, n_layers=1, n_heads=1, n_kv_heads=1, ffn_dim=128,
                        vocab_size=8, n_experts=4, top_k=2)
    layer = MoELayer(cfg)
    for p in layer.parameters():
        torch.nn.init.normal_(p, std=0.05)
    x, dout = torch.randn(2, 2, 64, 128).to(torch.bfloat16)
    return layer.to(torch.bfloat16), x, dout


def _run(layer, x, dout, ids=None):  # -> out, dx, weight grads as fp32; `ids` pins the routing
    x = x.detach().clone().requires_grad_()
    layer.zero_grad()
    if ids is None:
        out = layer(x)
    else:
        xt = x.reshape(-1, x.shape[-1])
        w = torch.softmax(torch.gather(layer.router(xt), 1, ids).float(), dim=-1).to(x.dtype)
        out = layer._dense_moe(xt, w, ids).reshape(x.shape)
    out.backward(dout)
    grads = [p.grad for ex in layer.experts for p in (ex.w13.weight, ex.w2.weight)]
    return [t.detach().float().cpu() for t in (out, x.grad, *grads)]


def test_grouped_matches_loop_and_fp32(monkeypatch):
    layer, x, dout = _layer_and_input()
    gpu = _layer_and_input()[0].cuda()  # the same seed: the same layer
    got = {}
    for backend in ("grouped", "loop"):
        monkeypatch.setenv("VESCALE_MOE_GEMM", backend)
        got[backend] = _run(gpu, x.cuda(), dout.cuda())
    ids = torch.topk(gpu.router(x.cuda().reshape(-1, 128)), 2, dim=-1)[1].cpu()
    monkeypatch.setenv("VESCALE_MOE_GEMM", "loop")
    ref = _run(layer.float(), x.float(), dout.float(), ids)
    for name, (g, l, r) in enumerate(zip(got["grouped"], got["loop"], ref)):  # out, dx, grads
        eg, el = float((g - r).abs().max()), float((l - r).abs().max())
        ulp = 2.0 ** (math.floor(math.log2(float(r.abs().max()))) - 7)
        print(f"tensor {name}: grouped err {eg:.3e}  loop err {el:.3e}  ulp {ulp:.3e}")
        assert eg <= 2 * el + ulp, name


def test_grouped_forward_has_no_host_sync(monkeypatch):
    layer, x = (t.cuda() for t in _layer_and_input()[:2])
    try:
        torch.cuda.set_sync_debug_mode("error")
        monkeypatch.setenv("VESCALE_MOE_GEMM", "grouped")
        with torch.no_grad():
            layer(x)
        monkeypatch.setenv("VESCALE_MOE_GEMM", "loop")
        with pytest.raises(RuntimeError), torch.no_grad():
            layer(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
