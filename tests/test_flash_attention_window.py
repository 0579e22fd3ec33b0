"""flash_attention(..., window=(left, right)) on the CPU path against a masked
softmax in fp64, the mask built from its definition around d(i) = i + shift:
j >= d(i) - left, j <= d(i) + right and, with is_causal, j <= d(i)."""
from dataclasses import replace

import pytest
import torch

from tests.test_flash_attention_segments import _no_intra_op_pool  # noqa: F401 (autouse: later files fork)
from vescale_amd.models import llama
from vescale_amd.ops import flash_attention


@pytest.mark.parametrize("Sq,Sk,shift", [(40, 40, 0), (12, 40, 28), (40, 12, 0)])
@pytest.mark.parametrize("causal", (True, False))
@pytest.mark.parametrize("left,right", [(0, 0), (5, None), (None, 3), (4, 2)])
def test_window_matches_dense_mask(left, right, causal, Sq, Sk, shift):
    g = torch.Generator().manual_seed(Sq + Sk)
    q, k, v = (torch.randn(2, h, s, 16, generator=g) for h, s in ((4, Sq), (2, Sk), (2, Sk)))
    o, lse = flash_attention(q, k, v, is_causal=causal, causal_shift=shift,
                             window=(left, right), return_lse=True)
    d = torch.arange(Sq)[:, None] + shift
    j = torch.arange(Sk)[None, :]
    vis = ((j >= d - (Sk + Sq if left is None else left))
           & (j <= d + (0 if causal else Sk + Sq if right is None else right)))
    dead = ~vis.any(-1)
    assert (Sq, Sk) != (40, 12) or left is None or dead[12 + left:].all()
    k, v = (t.double().repeat_interleave(2, dim=1) for t in (k, v))
    s = ((q.double() @ k.transpose(-1, -2)) / 4.0).masked_fill(~vis, -torch.inf)
    o64 = torch.softmax(s, -1).masked_fill(dead[:, None], 0.0) @ v
    assert (o[:, :, dead] == 0).all() and (lse[:, :, dead] == -torch.inf).all()
    torch.testing.assert_close(o.double(), o64, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(lse.double(), torch.logsumexp(s, -1), atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("window", [(-1, 0), (0, -2), (3,), (1, 2, 3), 5, (1.5, 0),
                                    (True, 0), ("4", None), None])
def test_bad_window_raises(window):     # None: causal_shift alone still needs is_causal
    q = torch.randn(1, 2, 8, 16)
    flash_attention(q, q, q, causal_shift=2, window=(3, 1))
    with pytest.raises(ValueError):
        flash_attention(q, q, q, causal_shift=2, window=window)


def test_model_sliding_window(monkeypatch):
    """sliding_window=W equals an explicit window=(W - 1, 0); full causal differs"""
    torch.manual_seed(0)
    cfg = replace(llama.llama_tiny(vocab=64, seq=32), sliding_window=5)
    model = llama.LlamaModel(cfg)
    model.init_weights()
    tokens = torch.randint(0, 64, (2, 24))
    y = model(tokens)
    cfg.sliding_window = None
    assert not torch.equal(model(tokens), y)
    monkeypatch.setattr(llama, "flash_attention_causal", lambda q, k, v: flash_attention(
        q, k, v, is_causal=True, window=(4, 0)))
    assert torch.equal(model(tokens), y)
    with pytest.raises(ValueError):
        llama.LlamaModel(replace(cfg, sliding_window=0))
