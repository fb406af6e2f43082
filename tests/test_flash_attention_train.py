"""The fused flash attention of training tenants (train_ops.FlashAttention,
ops.tenant.sdpa_lse / sdpa_bwd) on the CPU: the recompute-from-log-sum-exp
formulas the gfx950 kernels implement against fp64 autograd, the train spec's
``attention`` key, the memory estimate and a tiny decoder trained both ways.
The GPU twin (test_flash_attention_train_gpu.py) runs the kernels."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from nos_amd.ops import tenant as T
from nos_amd.podserver import train_ops


def _ref64(q, k, v, causal):
    """softmax(q k^T / sqrt(D)) v in fp64 autograd (grouped-query heads repeated)."""
    g = q.shape[2] // k.shape[2]
    k, v = k.repeat_interleave(g, 2), v.repeat_interleave(g, 2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / q.shape[-1] ** 0.5
    if causal:
        i = torch.arange(q.shape[1])[:, None] + (k.shape[1] - q.shape[1])
        s = s.masked_fill(torch.arange(k.shape[1])[None, :] > i, float("-inf"))
    return s, torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v)


def _grads(fn, *xs):
    xs = [x.detach().clone().requires_grad_(True) for x in xs]
    y = fn(*xs)
    g = torch.randn_like(y, generator=torch.Generator().manual_seed(7))
    y.backward(g)
    return y.detach(), [x.grad for x in xs]


def _qkv(g, sq, skv, B=2, hkv=2, D=16):
    torch.manual_seed(0)
    return (torch.randn(B, sq, hkv * g, D, dtype=torch.float64), torch.randn(B, skv, hkv, D, dtype=torch.float64),
            torch.randn(B, skv, hkv, D, dtype=torch.float64))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("g, sq, skv", [(1, 37, 37), (4, 70, 70), (2, 9, 40)])
def test_flash_attention_matches_fp64_autograd(causal, g, sq, skv):
    q, k, v = _qkv(g, sq, skv)
    y, gs = _grads(lambda a, b, c: train_ops.flash_attention(a, b, c, causal), q, k, v)
    y0, g0 = _grads(lambda a, b, c: _ref64(a, b, c, causal)[1], q, k, v)
    assert y.dtype == torch.float64
    torch.testing.assert_close(y, y0, rtol=1e-9, atol=1e-9)
    for a, b in zip(gs, g0):
        torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("causal", [False, True])
def test_reference_lse_is_the_logsumexp_of_the_masked_scores(causal):
    q, k, v = _qkv(2, 9, 40)
    s, o0 = _ref64(q, k, v, causal)
    o, lse = T.sdpa_lse_ref(q, k, v, causal)
    assert lse.shape == (2, 4, 9)
    torch.testing.assert_close(lse, torch.logsumexp(s, -1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(o, o0, rtol=1e-12, atol=1e-12)
    # the public ops take CPU tensors through the references
    o2, lse2 = T.sdpa_lse(q, k, v, causal)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)
    do = torch.randn_like(o)
    for a, b in zip(T.sdpa_bwd(q, k, v, o, lse, do, causal), T.sdpa_bwd_ref(q, k, v, o, lse, do, causal)):
        assert torch.equal(a, b)


def test_new_names_are_exported():
    for name in ("sdpa_lse", "sdpa_bwd", "sdpa_lse_ref", "sdpa_bwd_ref", "sdpa_bwd_workspace_bytes"):
        assert name in T.__all__ and callable(getattr(T, name))
    for name in ("FlashAttention", "flash_attention"):
        assert name in train_ops.__all__


def _llama(seq):
    from nos_amd.models.llama_program import llama_config, llama_model, llama_program
    from nos_amd.podserver import program as PG

    return PG.parse(*llama_program(llama_model(llama_config(False), 0), seq))


def test_train_spec_attention_key():
    from nos_amd.podserver.program import ProgramError
    from nos_amd.podserver.training import SPEC_KEYS, parse_train_spec

    p = _llama(16)
    assert "attention" in SPEC_KEYS
    assert parse_train_spec({"loss": "cross_entropy"}, p)["attention"] == "chunked"
    for a in ("chunked", "flash"):
        assert parse_train_spec({"loss": "cross_entropy", "attention": a}, p)["attention"] == a
    for bad in ("Flash", "sdpa", "", None, 1, True):
        with pytest.raises(ProgramError):
            parse_train_spec({"loss": "cross_entropy", "attention": bad}, p)


def test_flash_estimate_drops_the_live_scores_for_the_backward_workspace():
    """Per attention node both estimates count the saved log-sum-exp rows;
    "chunked" adds the live scores of the largest node's query chunk (in the
    doubled activation term), "flash" the largest backward workspace, once."""
    from nos_amd.podserver.training import parse_train_spec, train_bytes_estimate

    p = _llama(4096)
    est = {a: train_bytes_estimate(p, parse_train_spec({"loss": "cross_entropy", "optimizer": "adamw", "attention": a}, p))
           for a in ("chunked", "flash")}
    nodes = [n for n in p.nodes if n.op == "sdpa"]
    assert nodes
    live = ws = 0
    for n in nodes:
        (b, sq, h, d), (_, skv, hkv, _) = p.values[n.inputs[0]].shape, p.values[n.inputs[1]].shape
        live = max(live, train_ops.scores_bytes(b, h, sq, skv))
        ws = max(ws, T.sdpa_bwd_workspace_bytes(b, h, hkv, sq, skv, d))
    assert est["flash"] < est["chunked"]
    assert est["chunked"] - est["flash"] == 2 * live - ws


def test_tiny_decoder_trains_the_same_with_flash_and_chunked():
    from nos_amd.podserver.training import Trainer, parse_train_spec

    p = _llama(16)
    ids = np.random.default_rng(0).integers(0, 512, (1, 17)).astype(np.int64)
    losses = {}
    for a in ("flash", "chunked"):
        tr = Trainer(p, parse_train_spec({"loss": "cross_entropy", "optimizer": "adamw", "lr": 1e-2, "attention": a}, p),
                     "cpu")
        losses[a] = [float(tr.step(ids[:, :-1], ids[:, 1:])) for _ in range(3)]
    torch.testing.assert_close(torch.tensor(losses["flash"][0], dtype=torch.float32),
                               torch.tensor(losses["chunked"][0], dtype=torch.float32))
    for ls in losses.values():
        assert all(np.isfinite(ls)) and ls[-1] < ls[0]
