"""Int8 weight-only linears on gfx950 (csrc/hip/decode.hip ``gemv_q8_kernel``,
``dequant_q8_kernel``): the kernels against fp64 on the DEQUANTIZED weights
at the project's bar (4x torch-fp32's own error, at least 2e-6 of max |y|),
then the compiled int8 Llama tenant and the GPU pod server against
``dequantized_llama``."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402
from nos_amd.ops import _lib, _stream  # noqa: E402
from nos_amd.ops import tenant as T  # noqa: E402


@pytest.fixture(autouse=True)
def _h3():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)


def _weights(N: int, K: int, seed: int):
    """Full-range int8 rows: row 0 holds -128 and +127, row 1 is all zero, row 2 has a zero scale."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int32).to(torch.int8)
    sc = (torch.rand(N, generator=g) + 0.5) / (64.0 * K ** 0.5)
    q[0, 0], q[0, K - 1] = -128, 127
    if N > 1:
        q[1] = 0
    if N > 2:
        sc[2] = 0.0
    return q.cuda(), sc.cuda()


def _check(got, ref_args: tuple, ref_kw: dict, what) -> None:
    """got within max(4 e32, 2e-6) of the fp64 reference, relative to max |y|
    (e32: the same reference in torch fp32, on the same dequantized weights)."""
    ref64 = T.linear_q8_ref(*ref_args, **ref_kw, dtype=torch.float64)
    ref32 = T.linear_q8_ref(*ref_args, **ref_kw, dtype=torch.float32)
    scale = float(ref64.abs().max()) or 1.0
    e = float((got.double() - ref64).abs().max()) / scale
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    print(f"{what}: e = {e:.3g}, e32 = {e32:.3g}")
    assert got.shape == ref64.shape and e <= max(4 * e32, 2e-6), (what, e, e32)


# ------------------------------------------------------------------ 7. the GEMV
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("N, K", [(1, 16), (7, 48), (9, 1040), (1000, 1024), (64, 2816)])
def test_gemv_q8_matches_fp64(M, N, K):
    """K below one load batch, a K tail past 1024, odd N, a last partial
    column group, the down projection's K (three-load batches).  8 rows of
    K = 2816 are 88 KiB of x, over the kernel's 64 KiB of LDS: that one case
    is what ``linear_q8`` must route to the dequantize + h3 path, and is
    checked there at the same bar."""
    torch.manual_seed(M + N + K)
    q, sc = _weights(N, K, M + N + K)
    x = torch.randn(M, K, device="cuda")
    gamma = 1 + 0.1 * torch.randn(K, device="cuda")
    b = torch.randn(N, device="cuda")
    r = torch.randn(M, N, device="cuda")
    fits = M * K * 4 <= 65536
    assert T.gemv_q8_ok(x, q) == fits and (fits or (M, K) == (8, 2816))
    run = T.gemv_q8 if fits else T.linear_q8
    for act in (None, "gelu", "relu", "silu"):
        for bias, res in ((None, None), (b, r)):
            for kw in ({}, {"rms_eps": 1e-5, "gamma": gamma}):
                got = run(x, q, sc, bias, act, res, **kw)
                _check(got, (x, q, sc, bias, act, res), kw, (act, bias is not None, bool(kw)))


@pytest.mark.parametrize("M, N, K", [(1, 24616, 64), (3, 24616, 64), (1, 40, 4112), (3, 40, 4112)])
def test_gemv_q8_walks_several_groups_and_several_k_batches(M, N, K):
    """More column groups than workgroups (a vocabulary head: each workgroup
    walks two or three groups, the next one's weights prefetched), and a row
    longer than one batch of loads (K > 3072, with a one-lane tail block)."""
    torch.manual_seed(N + K)
    q, sc = _weights(N, K, N + K)
    x = torch.randn(M, K, device="cuda")
    gamma = 1 + 0.1 * torch.randn(K, device="cuda")
    b = torch.randn(N, device="cuda")
    r = torch.randn(M, N, device="cuda")
    for kw in ({}, {"rms_eps": 1e-5, "gamma": gamma}):
        _check(T.gemv_q8(x, q, sc, b, "gelu", r, **kw), (x, q, sc, b, "gelu", r), kw, bool(kw))


def test_gemv_q8_rms_prologue_without_gamma_and_strided_operands():
    """gamma = None is a gamma of ones; x rows and W rows may be strided (16-byte multiples)."""
    torch.manual_seed(0)
    q, sc = _weights(40, 256, 0)
    qs = torch.zeros(40, 512, dtype=torch.int8, device="cuda")
    qs[:, :256] = q
    xs = torch.randn(3, 512, device="cuda")
    x = xs[:, 128:384]
    assert T.gemv_q8_ok(x, qs[:, :256])
    got = T.gemv_q8(x, qs[:, :256], sc, rms_eps=1e-5)
    assert torch.equal(got, T.gemv_q8(x.contiguous(), q, sc, rms_eps=1e-5, gamma=torch.ones(256, device="cuda")))
    _check(got, (x, q, sc), {"rms_eps": 1e-5}, "strided")


# ------------------------------------------------------------------ 8. the GLU epilogue
@pytest.mark.parametrize("M", [1, 8])
def test_gemv_q8_glu_epilogue_matches_fp64(M):
    torch.manual_seed(M)
    K, Nh = 1024, 2816
    q, sc = _weights(2 * Nh, K, M)
    x = torch.randn(M, K, device="cuda")
    gamma = 1 + 0.1 * torch.randn(K, device="cuda")
    kw = {"rms_eps": 1e-5, "gamma": gamma, "glu": True}
    got = T.gemv_q8(x, q, sc, **kw)
    assert got.shape == (M, Nh)
    _check(got, (x, q, sc), kw, "glu")
    assert torch.equal(T.linear_q8(x.view(1, M, K), q, sc, **kw).view(M, Nh), got)


def test_gemv_q8_glu_odd_half_width():
    """Nh = 13: the last column group holds one gate / up pair for one wave only."""
    torch.manual_seed(1)
    q, sc = _weights(26, 64, 1)
    x = torch.randn(2, 64, device="cuda")
    _check(T.gemv_q8(x, q, sc, glu=True), (x, q, sc), {"glu": True}, "glu13")


# ------------------------------------------------------------------ 9. the decode partials
@pytest.mark.parametrize("D, B, G, Hkv", [(64, 1, 4, 2), (128, 2, 8, 1)])
def test_gemv_q8_combines_the_decode_partials(D, B, G, Hkv):
    L = 300
    torch.manual_seed(D + B + G + L)
    H = G * Hkv
    kc = torch.randn(B, L, Hkv, D, device="cuda")
    vc = torch.randn(B, L, Hkv, D, device="cuda")
    qq = torch.randn(B, 1, H, D, device="cuda")
    pos = torch.randint(0, L, (B,), dtype=torch.int32, device="cuda")
    pos[0] = L - 1
    N = 384
    wq, sc = _weights(N, H * D, D)
    bias = torch.randn(N, device="cuda")
    res = torch.randn(B, N, device="cuda")
    att = T.sdpa_cache(qq, kc, vc, pos).reshape(B, H * D)        # decode + attn_decode_combine
    want = T.gemv_q8(att, wq, sc, bias, None, res)
    p = T.sdpa_cache(qq, kc, vc, pos, partials=True)
    got = T.gemv_q8_partials(p, wq, sc, bias, None, res)
    assert torch.equal(got, want)
    _check(got, (att, wq, sc, bias, None, res), {}, "partials")


# ------------------------------------------------------------------ 10. dequantization
@pytest.mark.parametrize("N, K", [(7, 48), (1000, 1024)])
def test_dequant_q8_is_bit_exact(N, K):
    q, sc = _weights(N, K, N)
    got = T.dequant_q8(q, sc)
    assert got.dtype == torch.float32 and torch.equal(got, q.float() * sc[:, None])


# ------------------------------------------------------------------ 11. refusals
def _raw_gemv_q8(x, q, sc, y, M, N, K, epi=0) -> int:
    return _lib.lib().nos_gemv_q8(x.data_ptr(), x.stride(0), q.data_ptr(), q.stride(0), sc.data_ptr(), None, None, None,
                                  0, y.data_ptr(), y.stride(0), M, N, K, epi, 0.0, _stream())


@pytest.mark.parametrize("case", ["k-not-16", "nine-rows", "misaligned-w", "glu-odd-n"])
def test_gemv_q8_refuses_bad_arguments_without_a_launch(case):
    M, N, K, epi = 2, 8, 64, 0
    if case == "k-not-16":
        K = 56
    elif case == "nine-rows":
        M = 9
    elif case == "glu-odd-n":
        N, epi = 7, T.EPI_GLU
    x = torch.randn(M, 64, device="cuda")
    store = torch.ones(N * 64 + 16, dtype=torch.int8, device="cuda")
    off = 8 if case == "misaligned-w" else 0
    q = store[off:off + N * 64].view(N, 64)
    assert (q.data_ptr() % 16 != 0) == (case == "misaligned-w")
    sc = torch.ones(N, device="cuda")
    y = torch.full((M, N), 7.0, device="cuda")
    assert _raw_gemv_q8(x, q, sc, y, M, N, K, epi) != 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert not T.gemv_q8_ok(x[:, :K], q[:, :K]) or case == "glu-odd-n"


# ------------------------------------------------------------------ 12. routing
def test_nine_rows_route_to_the_dequantize_and_h3_path(monkeypatch):
    torch.manual_seed(9)
    q, sc = _weights(200, 256, 9)
    x = torch.randn(1, 9, 256, device="cuda")
    gamma = 1 + 0.1 * torch.randn(256, device="cuda")
    b = torch.randn(200, device="cuda")
    r = torch.randn(1, 9, 200, device="cuda")
    calls = []
    real = T.dequant_q8
    monkeypatch.setattr(T, "dequant_q8", lambda *a: (calls.append(1), real(*a))[1])
    monkeypatch.setattr(T, "gemv_q8", lambda *a, **k: pytest.fail("nine rows went to the GEMV"))
    for act in (None, "gelu", "relu", "silu"):
        for bias, res in ((None, None), (b, r)):
            for kw in ({}, {"rms_eps": 1e-5, "gamma": gamma}):
                got = T.linear_q8(x, q, sc, bias, act, res, **kw)
                _check(got, (x, q, sc, bias, act, res), kw, (act, bias is not None, bool(kw)))
    assert len(calls) == 16        # dequantized on every call: the fp32 weight is a transient, never cached


# ------------------------------------------------------------------ whole tenants
@pytest.fixture(scope="module")
def model():
    from nos_amd.models.llama_program import llama_config, llama_model

    return llama_model(llama_config(False), 0)


@pytest.fixture(scope="module")
def deq(model):
    from nos_amd.models.llama_program import dequantized_llama

    return dequantized_llama(model)


def _compiled(model, weights: str, prompt_len: int = 8, max_len: int = 128):
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    progs, w = llama_decode_programs(model, prompt_len, max_len, weights=weights)
    ps = PG.parse_variants(progs, w, gpu=True)
    params = ps[0].tensors("cuda")
    state = ps[0].state_tensors("cuda")
    return [p.compile("cuda", params=params, state=state) for p in ps], state


def test_int8_decode_step_logits_match_the_dequantized_model_in_fp64(model, deq):
    """13. Prefill 8 (8 rows: the GEMV) + 3 decode steps compiled for the GPU."""
    import copy

    (pre, step), state = _compiled(model, "int8")
    prompt = torch.randint(0, model.config.vocab_size, (1, 8), device="cuda")
    seq = prompt.clone()
    with torch.no_grad():
        logits, nxt = pre(prompt.int())
        for _ in range(3):
            seq = torch.cat([seq, nxt.long().view(1, 1)], 1)
            logits, nxt = step(nxt.view(1, 1).int())
        mc = copy.deepcopy(deq).cuda()
        f32 = mc(seq).logits[:, -1:]
        ref64 = mc.double()(seq).logits[:, -1:]
    e = float((logits.double() - ref64).abs().max() / ref64.abs().max())
    e32 = float((f32.double() - ref64).abs().max() / ref64.abs().max())
    print(f"e = {e:.3g}, e32 = {e32:.3g}")
    assert e <= max(4 * e32, 1e-5), (e, e32)
    assert state["pos"].tolist() == [11]


def test_int8_prefill_over_eight_rows_takes_the_h3_path_and_matches(model, deq):
    """A 16-token prefill: every linear_q8 but the one-row head dequantizes into a transient."""
    import copy

    (pre, _), state = _compiled(model, "int8", prompt_len=16)
    prompt = torch.randint(0, model.config.vocab_size, (1, 16), device="cuda")
    with torch.no_grad():
        logits, _ = pre(prompt.int())
        mc = copy.deepcopy(deq).cuda()
        f32 = mc(prompt).logits[:, -1:]
        ref64 = mc.double()(prompt).logits[:, -1:]
    e = float((logits.double() - ref64).abs().max() / ref64.abs().max())
    e32 = float((f32.double() - ref64).abs().max() / ref64.abs().max())
    print(f"e = {e:.3g}, e32 = {e32:.3g}")
    assert e <= max(4 * e32, 1e-5), (e, e32)
    assert state["pos"].tolist() == [16]


def test_int8_decode_step_keeps_every_fusion_of_the_fp32_step(model):
    """14."""
    (_, q8), _ = _compiled(model, "int8")
    (_, f32), _ = _compiled(model, "fp32")
    layers = model.config.num_hidden_layers
    assert f32.stats["rmsnorm_folded"] == 2 * layers + 1     # the decode step's linears behind a norm
    assert q8.stats["q8_rms_prologue"] == f32.stats["rmsnorm_folded"]
    assert q8.stats["q8_glu_fused"] == f32.stats["gemv_glu_fused"] == layers
    assert q8.stats["q8_combines_into_gemv"] == f32.stats["decode_combines_into_gemv"] == layers
    assert q8.stats["q8_linears"] == 4 * layers + 1
    assert q8.stats["kernels"] <= f32.stats["kernels"]
    kinds = [s.kind for s in q8.steps]
    assert "linear" not in kinds and "glu" not in kinds and "rmsnorm" not in kinds and "linear_rms" not in kinds
    assert all(t.dtype != torch.float32 or t.dim() != 2 or k.startswith(("rope.", "model.embed"))
               for k, t in q8.consts.items()), "no fp32 copy of a quantized weight"


def test_gpu_server_generates_the_dequantized_models_tokens(model, deq, tmp_path):
    """15. HIP graphs and the server loop; a second sequence after reset() repeats the first."""
    import copy

    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    PROMPT_LEN, NEW, MAX_LEN = 16, 32, 64

    def _prompt():   # seed 2: the fp64 reference's top-2 gap clears 1e-4 at every step (asserted)
        return np.random.default_rng(2).integers(0, 512, (1, PROMPT_LEN)).astype(np.int32)

    m64 = copy.deepcopy(deq).double()
    seq = torch.from_numpy(_prompt().astype(np.int64))
    gap = float("inf")
    with torch.no_grad():
        for _ in range(NEW):   # greedy, in fp64, on the dequantized weights alone
            logits = m64(seq).logits[0, -1]
            top = logits.topk(2)
            gap = min(gap, float((top.values[0] - top.values[1]) / logits.abs().max()))
            seq = torch.cat([seq, top.indices[:1].view(1, 1)], 1)
    assert gap >= 1e-4, gap
    want = deq.generate(torch.from_numpy(_prompt().astype(np.int64)), max_new_tokens=NEW, min_new_tokens=NEW,
                        do_sample=False, pad_token_id=0)[:, PROMPT_LEN:].numpy()
    assert np.array_equal(seq[:, PROMPT_LEN:].numpy(), want)
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="int8")
    srv = PodServer(tmp_path / "g.sock", device="cuda", lanes=2, memory_gb=40).start()
    try:
        c = PodClient(srv.path, connect_timeout_s=60)
        c.register("llm-q8", progs[0], w, memory_limit_gb=4, variants=progs[1:])
        ids, tm = c.generate(_prompt(), NEW, server_loop=True)
        assert np.array_equal(ids, want), (ids, want)
        assert tm["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
        c.reset()
        again, tm2 = c.generate(_prompt(), NEW, server_loop=True)
        assert np.array_equal(again, want) and tm2["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
        c.close()
    finally:
        srv.stop()
