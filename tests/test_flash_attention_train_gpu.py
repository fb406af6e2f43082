"""The fused flash attention of training tenants on the gfx950 kernels
(csrc/hip/attention_h3g.hip ``nos_attn_h3g_lse``, attention_h3g_bwd.hip):
the forward is the inference kernel bit for bit and adds the rows'
log-sum-exp; the backward against fp64 autograd under the criterion of
test_train_ops_gpu.py (``rel <= max(4 rel(torch fp32), 1e-5)``), through
strides, under badly scaled rows, bit-reproducible, graph-captured, and as a
training tenant's attention."""
from __future__ import annotations

import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd.ops import _lib, tenant as T  # noqa: E402
from nos_amd.podserver import train_ops  # noqa: E402

B, HKV = 2, 2
SHAPES = [(1, 1, 1), (1, 33, 33), (4, 300, 300), (2, 40, 300), (4, 1100, 1100)]   # (g, Sq, Skv)


def _ref(q, k, v, causal):
    g = q.shape[2] // k.shape[2]
    k, v = k.repeat_interleave(g, 2), v.repeat_interleave(g, 2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / q.shape[-1] ** 0.5
    if causal:
        i = torch.arange(q.shape[1], device=q.device)[:, None] + (k.shape[1] - q.shape[1])
        s = s.masked_fill(torch.arange(k.shape[1], device=q.device)[None, :] > i, float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v)


def _autograd(q, k, v, do, causal):
    xs = [x.detach().clone().requires_grad_(True) for x in (q, k, v)]
    y = _ref(*xs, causal)
    y.backward(do.to(y.dtype))
    return [y.detach()] + [x.grad for x in xs]


def _rel(a, b, zero_den: float) -> float:
    """max|a - b| / max|b|.  Where the fp64 reference is identically zero (one
    key: dS = P (dP - delta) cancels exactly, so dq = dk = 0) that ratio is
    undefined; the error is then taken relative to the terms that cancel:
    scale max|dP| max|K or Q| (``zero_den``)."""
    den = float(b.double().abs().max())
    return float((a.double() - b.double()).abs().max()) / (den if den > 0 else zero_den)


def _zero_dens(q, k, v, do):
    """Per output (o, dq, dk, dv): the magnitude of the cancelling terms of dq / dk."""
    g = q.shape[2] // k.shape[2]
    dp = torch.einsum("bqhd,bkhd->bhqk", do.double(), v.double().repeat_interleave(g, 2)).abs().max()
    sc = q.shape[-1] ** -0.5
    return [1.0, float(sc * dp * k.abs().max()), float(sc * dp * q.abs().max()), 1.0]


def _inputs(D, g, sq, skv, seed=0):
    gen = torch.Generator(device="cuda").manual_seed(seed + 131 * D + 7 * g + sq + skv)
    return (torch.randn(B, sq, HKV * g, D, device="cuda", generator=gen),
            torch.randn(B, skv, HKV, D, device="cuda", generator=gen),
            torch.randn(B, skv, HKV, D, device="cuda", generator=gen),
            torch.randn(B, sq, HKV * g, D, device="cuda", generator=gen))


@functools.lru_cache(maxsize=None)
def _case(D, causal, g, sq, skv):
    """Inputs, the fp64 and the torch-fp32 autograd results: computed once, shared, never written."""
    q, k, v, do = _inputs(D, g, sq, skv)
    r64 = _autograd(q.double(), k.double(), v.double(), do.double(), causal)
    r32 = _autograd(q, k, v, do, causal)
    return (q, k, v, do), r64, r32


def _check(ours, r64, r32, dens):
    for name, a, b, c, zd in zip(("o", "dq", "dk", "dv"), ours, r64, r32, dens):
        assert torch.isfinite(a).all(), name
        ea, ec = _rel(a, b, zd), _rel(c, b, zd)
        print(f"{name}: rel(ours) {ea:.3e}  rel(torch fp32) {ec:.3e}")
        assert ea <= max(4 * ec, 1e-5), (name, ea, ec)


def _fwd_bwd(q, k, v, do, causal):
    o, lse = T.sdpa_lse(q, k, v, causal)
    return (o, *T.sdpa_bwd(q, k, v, o, lse, do, causal)), lse


# ------------------------------------------------------------------ forward
def test_forward_is_sdpa_bit_for_bit_and_adds_the_log_sum_exp():
    gen = torch.Generator(device="cuda").manual_seed(3)
    q = torch.randn(1, 300, 4, 128, device="cuda", generator=gen)
    k = torch.randn(1, 300, 2, 128, device="cuda", generator=gen)
    v = torch.randn(1, 300, 2, 128, device="cuda", generator=gen)
    s64 = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double().repeat_interleave(2, 2)) / 128 ** 0.5
    mask = torch.arange(300, device="cuda")[None, :] > torch.arange(300, device="cuda")[:, None]
    l64 = torch.logsumexp(s64.masked_fill(mask, float("-inf")), -1)
    s32 = torch.einsum("bqhd,bkhd->bhqk", q, k.repeat_interleave(2, 2)) / 128 ** 0.5
    err32 = float((torch.logsumexp(s32.masked_fill(mask, float("-inf")), -1).double() - l64).abs().max())
    try:
        for split in (0, 2):
            T.set_attention_h3g_kvsplit(split)
            o, lse = T.sdpa_lse(q, k, v, causal=True)
            assert torch.equal(o, T.sdpa(q, k, v, causal=True)), split
            assert lse.shape == (1, 4, 300) and lse.dtype == torch.float32
            err = float((lse.double() - l64).abs().max())
            print(f"kvsplit {split}: lse err {err:.3e}  torch fp32 {err32:.3e}")
            assert err <= max(4 * err32, 1e-5), (split, err, err32)
    finally:
        T.set_attention_h3g_kvsplit(0)


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("g, sq, skv", SHAPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_backward_matches_fp64(D, causal, g, sq, skv):
    (q, k, v, do), r64, r32 = _case(D, causal, g, sq, skv)
    ours, _ = _fwd_bwd(q, k, v, do, causal)
    _check(ours, r64, r32, _zero_dens(q, k, v, do))


def test_autograd_function_on_gpu_matches_fp64():
    """train_ops.flash_attention end to end (forward, saved tensors, backward)."""
    (q, k, v, do), r64, r32 = _case(128, True, 4, 300, 300)
    xs = [x.detach().clone().requires_grad_(True) for x in (q, k, v)]
    y = train_ops.flash_attention(*xs, True)
    y.backward(do)
    _check([y.detach()] + [x.grad for x in xs], r64, r32, _zero_dens(q, k, v, do))


def test_strided_views_give_the_contiguous_results():
    """q / k / v as slices of one fused projection and a non-contiguous dO."""
    g, S, D = 4, 300, 128
    H = HKV * g
    gen = torch.Generator(device="cuda").manual_seed(5)
    qkv = torch.randn(B, S, (H + 2 * HKV) * D, device="cuda", generator=gen)
    q = qkv[..., :H * D].view(B, S, H, D)
    k = qkv[..., H * D:(H + HKV) * D].view(B, S, HKV, D)
    v = qkv[..., (H + HKV) * D:].view(B, S, HKV, D)
    do = torch.randn(B, H, S, D, device="cuda", generator=gen).permute(0, 2, 1, 3)   # heads not contiguous per token
    do2 = torch.randn(B, S, 2 * H * D, device="cuda", generator=gen)[..., :H * D].view(B, S, H, D)   # a strided view
    assert not q.is_contiguous() and not do.is_contiguous() and not do2.is_contiguous()
    for d in (do, do2):
        a, la = _fwd_bwd(q, k, v, d, True)
        b, lb = _fwd_bwd(q.contiguous(), k.contiguous(), v.contiguous(), d.contiguous(), True)
        assert torch.equal(la, lb)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_scale_rule_badly_scaled_rows_and_heads():
    """One query row, one dO row and one key 1e3 times larger, one query head
    1e-3 times smaller: a per-row scale used inside a reduction over rows, or
    an unbounded dS, would show here."""
    (q, k, v, do), _, _ = _case(128, True, 4, 300, 300)
    q, k, do = q.clone(), k.clone(), do.clone()
    q[0, 17, 1] *= 1e3
    do[1, 211, 5] *= 1e3
    k[0, 100, 1] *= 1e3
    q[:, :, 6] *= 1e-3
    r64 = _autograd(q.double(), k.double(), v.double(), do.double(), True)
    r32 = _autograd(q, k, v, do, True)
    ours, _ = _fwd_bwd(q, k, v, do, True)
    _check(ours, r64, r32, _zero_dens(q, k, v, do))


def test_backward_is_bit_reproducible_and_needs_no_zeroed_outputs():
    (q, k, v, do), _, _ = _case(128, True, 4, 1100, 1100)
    o, lse = T.sdpa_lse(q, k, v, True)
    runs = []
    for _ in range(2):
        out = tuple(torch.full_like(t, float("nan")) for t in (q, k, v))
        T.sdpa_bwd(q, k, v, o, lse, do, True, out=out)
        runs.append(out)
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    for a, b in zip(runs[0], T.sdpa_bwd(q, k, v, o, lse, do, True)):
        assert torch.equal(a, b)


def test_forward_and_backward_replay_in_a_graph():
    """Captured once, replayed on new inputs: every replay equals its own
    eager result (no state of the capture's inputs survives in a workspace)."""
    D, g, S = 128, 4, 300
    static = [t.clone() for t in _inputs(D, g, S, S, seed=1)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _fwd_bwd(*static, True)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs, lse = _fwd_bwd(*static, True)
    for seed in (2, 3):
        fresh = _inputs(D, g, S, S, seed=seed)
        for s, f in zip(static, fresh):
            s.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        eager, elle = _fwd_bwd(*fresh, True)
        assert torch.equal(lse, elle)
        for a, b in zip(outs, eager):
            assert torch.equal(a, b), seed


def test_workspace_formula_and_a_short_workspace_is_refused():
    L = _lib.lib()
    for D, (g, sq, skv) in itertools.product((64, 128), SHAPES):
        assert T.sdpa_bwd_workspace_bytes(B, HKV * g, HKV, sq, skv, D) == \
            int(L.nos_attn_h3g_bwd_workspace(B, HKV * g, HKV, sq, skv, D))
    D, g, S = 64, 1, 33
    q, k, v, do = _inputs(D, g, S, S)
    o, lse = T.sdpa_lse(q, k, v, True)
    n = T.sdpa_bwd_workspace_bytes(B, HKV * g, HKV, S, S, D)
    ws = torch.empty(n + 256, dtype=torch.uint8, device="cuda")
    wptr = (ws.data_ptr() + 255) // 256 * 256
    outs = [torch.full_like(t, float("nan")) for t in (q, k, v)]

    def call(nbytes):
        ld, ldk = HKV * g * D, HKV * D
        return L.nos_attn_h3g_bwd(q.data_ptr(), ld, S * ld, k.data_ptr(), ldk, S * ldk, v.data_ptr(), ldk, S * ldk,
                                  o.data_ptr(), ld, S * ld, do.data_ptr(), ld, S * ld, lse.data_ptr(),
                                  outs[0].data_ptr(), ld, S * ld, outs[1].data_ptr(), ldk, S * ldk, outs[2].data_ptr(),
                                  ldk, S * ldk, B, HKV * g, HKV, S, S, D, 1, D ** -0.5, wptr, nbytes,
                                  torch.cuda.current_stream().cuda_stream)

    assert call(n - 1) == 1                      # hipErrorInvalidValue, nothing launched:
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in outs)
    assert call(n) == 0
    torch.cuda.synchronize()
    for a, b in zip(outs, T.sdpa_bwd(q, k, v, o, lse, do, True)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ tenant
def test_decoder_fine_tune_with_flash_attention(tmp_path):
    """The small Llama of the seq-2048 test, registered with the flash and
    with the chunked attention.  At seq 512 (short): flash trains, and its
    first loss is the chunked tenant's (both fp32-class forwards of the same
    weights).  The measured footprints are compared at seq 2048, that test's
    own length: at seq 512 the peak of either tenant is the AdamW step
    (weights + gradients + two moments + its temporaries, ~3.6 GB), which no
    attention changes -- three processes measured flash / chunked 3.605 /
    3.607, 3.616 / 3.614 and 3.619 / 3.626 GB there, allocator noise -- while
    at seq 2048 the activations are part of the peak (4.368 against 4.427 GB)."""
    from nos_amd.models.llama_program import llama_config, llama_model, llama_program
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    model = llama_model(llama_config(True), 0)
    spec = {"loss": "cross_entropy", "optimizer": "adamw", "lr": 1e-4}
    srv = PodServer(tmp_path / "t.sock", device="cuda", lanes=2, memory_gb=64).start()
    try:
        prog, w = llama_program(model, 512)
        ids = np.random.default_rng(0).integers(0, 32000, (1, 513)).astype(np.int32)
        cl = {a: PodClient(srv.path, connect_timeout_s=60) for a in ("flash", "chunked")}
        for a, c in cl.items():
            c.register(a, prog, w, memory_limit_gb=10, train={**spec, "attention": a})
        losses = [cl["flash"].train_step(ids[:, :-1], ids[:, 1:])["loss"] for _ in range(3)]
        first = cl["chunked"].train_step(ids[:, :-1], ids[:, 1:])["loss"]
        print("flash", losses, "chunked", first)
        assert all(np.isfinite(losses)) and losses[-1] < losses[1] < losses[0]
        np.testing.assert_allclose(losses[0], first, rtol=1e-5)
        for c in cl.values():
            c.close()
        prog, w = llama_program(model, 2048)
        foot = {}
        for a in ("flash", "chunked"):
            c = PodClient(srv.path, connect_timeout_s=60)
            foot[a] = c.register(a + "-2048", prog, w, memory_limit_gb=10, train={**spec, "attention": a})["footprint_gb"]
            c.close()
        print("footprint_gb at seq 2048", foot)
        assert foot["flash"] < foot["chunked"] < 10
    finally:
        srv.stop()
