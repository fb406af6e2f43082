"""MXFP4 weight-only linears on gfx950 (csrc/hip/decode.hip ``gemv_mx4_kernel``,
``dequant_mx4_kernel``): the conversion bit for bit against
``dequantize_rows_mx4``, the kernels against fp64 on the DEQUANTIZED weights
at the project's bar (4x torch-fp32's own error, at least 2e-6 of max |y|),
then the compiled MXFP4 Llama tenant and the GPU pod server against
``dequantized_llama(model, "mxfp4")``."""
from __future__ import annotations

import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402
from nos_amd.ops import _lib, _stream  # noqa: E402
from nos_amd.ops import tenant as T  # noqa: E402
from nos_amd.podserver.program import dequantize_rows_mx4  # noqa: E402


@pytest.fixture(autouse=True)
def _h3():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)


def _weights(N: int, K: int, seed: int):
    """Random nibbles over all 16 codes (both zeros, 0x0 and 0x8, among them), row 1 all zero, block
    scales random in 127 +- 6 lowered by about log2(sqrt K) so that y stays O(1)."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    if N > 1:
        codes[1] = 0
    off = int(round(math.log2(math.sqrt(K)))) + 1
    sc = (torch.randint(121, 134, (N, K // 32), generator=g, dtype=torch.int32) - off).to(torch.uint8)
    return codes.cuda(), sc.cuda()


def _check(got, ref_args: tuple, ref_kw: dict, what) -> None:
    """got within max(4 e32, 2e-6) of the fp64 reference, relative to max |y|
    (e32: the same reference in torch fp32, on the same dequantized weights)."""
    ref64 = T.linear_mx4_ref(*ref_args, **ref_kw, dtype=torch.float64)
    ref32 = T.linear_mx4_ref(*ref_args, **ref_kw, dtype=torch.float32)
    scale = float(ref64.abs().max()) or 1.0
    e = float((got.double() - ref64).abs().max()) / scale
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    print(f"{what}: e = {e:.3g}, e32 = {e32:.3g}")
    assert got.shape == ref64.shape and e <= max(4 * e32, 2e-6), (what, e, e32)


# ------------------------------------------------------------------ the conversion, bit for bit
def _every_code_weights(N: int, K: int):
    """Every code in both nibble positions under each of the scale bytes 2, 126, 127, 128, 252."""
    i = torch.arange(N * (K // 2), dtype=torch.int64).view(N, K // 2)
    blk, p = i // 16, i % 16                       # within each block of 16 bytes both nibbles walk 0 .. 15
    codes = (((p + blk) % 16) | (((5 * p + 3 + blk) % 16) << 4)).to(torch.uint8)
    j = torch.arange(N * (K // 32), dtype=torch.int64).view(N, K // 32)
    sc = torch.tensor([2, 126, 127, 128, 252], dtype=torch.uint8)[(j + j // (K // 32)) % 5]
    return codes, sc


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("N, K", [(7, 96), (1000, 1024)])
def test_dequant_mx4_is_bit_exact_and_is_what_the_gemv_multiplies(N, K):
    codes, sc = _every_code_weights(N, K)
    want = torch.from_numpy(dequantize_rows_mx4(codes.numpy(), sc.numpy()))
    for s in (2, 126, 127, 128, 252):     # every (code, scale) pair is present, in both nibbles
        for nib in (codes & 15, codes >> 4):
            rows = nib[(sc == s).repeat_interleave(16, dim=1)]
            assert set(rows.tolist()) == set(range(16)), (s, sorted(set(rows.tolist())))
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) == 6.0 * 2.0 ** 125
    nz = want[want != 0].abs()
    assert float(nz.min()) == 0.5 * 2.0 ** -125 and float(nz.min()) >= torch.finfo(torch.float32).tiny
    got = T.dequant_mx4(codes.cuda(), sc.cuda())
    assert got.dtype == torch.float32 and got.shape == (N, K)
    assert torch.equal(_bits(got).cpu(), _bits(want)), "dequant_mx4 differs from dequantize_rows_mx4"
    assert torch.equal(_bits(T.dequant_mx4(codes, sc)), _bits(want))       # the CPU path, too
    # a one-hot x at M = 1: y[n] is W[n, k] itself (one product by 1.0, zeros elsewhere), exactly
    cg, sg = codes.cuda(), sc.cuda()
    for k in sorted({0, 1, 2, 5, 30, 31, 32, 33, K // 2 - 1, K // 2, K - 34, K - 2, K - 1}):
        x = torch.zeros(1, K, device="cuda")
        x[0, k] = 1.0
        y = T.gemv_mx4(x, cg, sg)[0].cpu()
        assert torch.equal(y, want[:, k]), (k, y[:4], want[:4, k])


# ------------------------------------------------------------------ the GEMV
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("N, K", [(1, 32), (7, 96), (9, 2080), (1000, 1024), (64, 2816)])
def test_gemv_mx4_matches_fp64(M, N, K):
    """K of one block (below one load), a K tail past one wave load (2048 + 32), odd N, a last
    partial column group, the down projection's K (two-load batches).  8 rows of K = 2816 are 88 KiB
    of x and 8 rows of K = 2080 are 65 KiB, over the kernel's 64 KiB of LDS: those cases are what
    ``linear_mx4`` must route to the dequantize + h3 path, and are checked there at the same bar."""
    torch.manual_seed(M + N + K)
    q, sc = _weights(N, K, M + N + K)
    x = torch.randn(M, K, device="cuda")
    gamma = 1 + 0.1 * torch.randn(K, device="cuda")
    b = torch.randn(N, device="cuda")
    r = torch.randn(M, N, device="cuda")
    fits = M * K * 4 <= 65536
    assert T.gemv_mx4_ok(x, q) == fits and (fits or (M, K) in ((8, 2080), (8, 2816)))
    run = T.gemv_mx4 if fits else T.linear_mx4
    for act in (None, "gelu", "relu", "silu"):
        for bias, res in ((None, None), (b, r)):
            for kw in ({}, {"rms_eps": 1e-5, "gamma": gamma}):
                got = run(x, q, sc, bias, act, res, **kw)
                _check(got, (x, q, sc, bias, act, res), kw, (act, bias is not None, bool(kw)))


@pytest.mark.parametrize("M, N, K", [(1, 24616, 64), (3, 24616, 64), (1, 40, 4128), (3, 40, 4128), (1, 40, 1056)])
def test_gemv_mx4_walks_several_groups_and_several_k_batches(M, N, K):
    """More column groups than workgroups (a vocabulary head: each workgroup walks two or three
    groups, the next one's weights prefetched); a row longer than one batch of loads (the kernel as
    built takes 2 x 2048 k per batch: K = 4128 is a second batch of a one-lane tail block); and the
    first K past the 8-byte-load form's 1024."""
    torch.manual_seed(N + K)
    q, sc = _weights(N, K, N + K)
    x = torch.randn(M, K, device="cuda")
    gamma = 1 + 0.1 * torch.randn(K, device="cuda")
    b = torch.randn(N, device="cuda")
    r = torch.randn(M, N, device="cuda")
    for kw in ({}, {"rms_eps": 1e-5, "gamma": gamma}):
        _check(T.gemv_mx4(x, q, sc, b, "gelu", r, **kw), (x, q, sc, b, "gelu", r), kw, bool(kw))


def test_gemv_mx4_rms_prologue_without_gamma_and_strided_operands():
    """gamma = None is a gamma of ones; x, the codes' and the scales' rows, the residual and y's
    source may be strided."""
    torch.manual_seed(0)
    q, sc = _weights(40, 256, 0)
    qs = torch.zeros(40, 256, dtype=torch.uint8, device="cuda")
    qs[:, :128] = q
    ss = torch.zeros(40, 24, dtype=torch.uint8, device="cuda")
    ss[:, :8] = sc
    xs = torch.randn(3, 512, device="cuda")
    x = xs[:, 128:384]
    rs = torch.randn(3, 80, device="cuda")
    r = rs[:, 8:48]
    assert T.gemv_mx4_ok(x, qs[:, :128]) and not r.is_contiguous()
    got = T.gemv_mx4(x, qs[:, :128], ss[:, :8], residual=r, rms_eps=1e-5)
    want = T.gemv_mx4(x.contiguous(), q, sc, residual=r.contiguous(), rms_eps=1e-5, gamma=torch.ones(256, device="cuda"))
    assert torch.equal(got, want)
    _check(got, (x, q, sc, None, None, r), {"rms_eps": 1e-5}, "strided")


# ------------------------------------------------------------------ the GLU epilogue
@pytest.mark.parametrize("M", [1, 8])
def test_gemv_mx4_glu_epilogue_matches_fp64(M):
    torch.manual_seed(M)
    K, Nh = 1024, 2816
    q, sc = _weights(2 * Nh, K, M)
    x = torch.randn(M, K, device="cuda")
    gamma = 1 + 0.1 * torch.randn(K, device="cuda")
    kw = {"rms_eps": 1e-5, "gamma": gamma, "glu": True}
    got = T.gemv_mx4(x, q, sc, **kw)
    assert got.shape == (M, Nh)
    _check(got, (x, q, sc), kw, "glu")
    assert torch.equal(T.linear_mx4(x.view(1, M, K), q, sc, **kw).view(M, Nh), got)


def test_gemv_mx4_glu_odd_half_width():
    """Nh = 13: the last column group holds one gate / up pair for one wave only."""
    torch.manual_seed(1)
    q, sc = _weights(26, 64, 1)
    x = torch.randn(2, 64, device="cuda")
    _check(T.gemv_mx4(x, q, sc, glu=True), (x, q, sc), {"glu": True}, "glu13")


# ------------------------------------------------------------------ the decode partials
@pytest.mark.parametrize("D, B, G, Hkv", [(64, 1, 4, 2), (128, 2, 8, 1)])
def test_gemv_mx4_combines_the_decode_partials(D, B, G, Hkv):
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
    want = T.gemv_mx4(att, wq, sc, bias, None, res)
    p = T.sdpa_cache(qq, kc, vc, pos, partials=True)
    got = T.gemv_mx4_partials(p, wq, sc, bias, None, res)
    assert torch.equal(got, want)
    _check(got, (att, wq, sc, bias, None, res), {}, "partials")


# ------------------------------------------------------------------ refusals
def _raw_gemv_mx4(x, q, sc, y, M, N, K, epi=0) -> int:
    return _lib.lib().nos_gemv_mx4(x.data_ptr(), x.stride(0), q.data_ptr(), q.stride(0), sc.data_ptr(), sc.stride(0),
                                   None, None, None, 0, y.data_ptr(), y.stride(0), M, N, K, epi, 0.0, _stream())


@pytest.mark.parametrize("case", ["k-not-32", "nine-rows", "misaligned-w", "glu-odd-n"])
def test_gemv_mx4_refuses_bad_arguments_without_a_launch(case):
    M, N, K, epi = 2, 8, 128, 0
    if case == "k-not-32":
        K = 112
    elif case == "nine-rows":
        M = 9
    elif case == "glu-odd-n":
        N, epi = 7, T.EPI_GLU
    x = torch.randn(M, 128, device="cuda")
    store = torch.ones(N * 64 + 16, dtype=torch.uint8, device="cuda")
    off = 8 if case == "misaligned-w" else 0
    q = store[off:off + N * 64].view(N, 64)
    assert (q.data_ptr() % 16 != 0) == (case == "misaligned-w")
    sc = torch.full((N, 4), 127, dtype=torch.uint8, device="cuda")
    y = torch.full((M, N), 7.0, device="cuda")
    assert _raw_gemv_mx4(x, q, sc, y, M, N, K, epi) != 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert not T.gemv_mx4_ok(x[:, :K], q[:, :K // 2]) or case == "glu-odd-n"
    with pytest.raises(ValueError):
        T.gemv_mx4(x[:, :K], q[:, :K // 2], sc[:, :max(K // 32, 1)], glu=bool(epi))


# ------------------------------------------------------------------ routing
def test_nine_rows_route_to_the_dequantize_and_h3_path(monkeypatch):
    torch.manual_seed(9)
    q, sc = _weights(200, 256, 9)
    x = torch.randn(1, 9, 256, device="cuda")
    gamma = 1 + 0.1 * torch.randn(256, device="cuda")
    b = torch.randn(200, device="cuda")
    r = torch.randn(1, 9, 200, device="cuda")
    calls = []
    real = T.dequant_mx4
    monkeypatch.setattr(T, "dequant_mx4", lambda *a: (calls.append(1), real(*a))[1])
    monkeypatch.setattr(T, "gemv_mx4", lambda *a, **k: pytest.fail("nine rows went to the GEMV"))
    for act in (None, "gelu", "relu", "silu"):
        for bias, res in ((None, None), (b, r)):
            for kw in ({}, {"rms_eps": 1e-5, "gamma": gamma}):
                got = T.linear_mx4(x, q, sc, bias, act, res, **kw)
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

    return dequantized_llama(model, weights="mxfp4")


def _compiled(model, weights: str, prompt_len: int = 8, max_len: int = 128):
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    progs, w = llama_decode_programs(model, prompt_len, max_len, weights=weights)
    ps = PG.parse_variants(progs, w, gpu=True)
    params = ps[0].tensors("cuda")
    state = ps[0].state_tensors("cuda")
    return [p.compile("cuda", params=params, state=state) for p in ps], state


def _logit_errors(logits, deq, seq):
    with torch.no_grad():
        mc = copy.deepcopy(deq).cuda()
        f32 = mc(seq).logits[:, -1:]
        ref64 = mc.double()(seq).logits[:, -1:]
    e = float((logits.double() - ref64).abs().max() / ref64.abs().max())
    e32 = float((f32.double() - ref64).abs().max() / ref64.abs().max())
    print(f"e = {e:.3g}, e32 = {e32:.3g}")
    return e, e32


def test_mxfp4_decode_step_logits_match_the_dequantized_model_in_fp64(model, deq):
    """Prefill 8 (8 rows: the GEMV) + 3 decode steps compiled for the GPU."""
    (pre, step), state = _compiled(model, "mxfp4")
    prompt = torch.randint(0, model.config.vocab_size, (1, 8), device="cuda")
    seq = prompt.clone()
    with torch.no_grad():
        logits, nxt = pre(prompt.int())
        for _ in range(3):
            seq = torch.cat([seq, nxt.long().view(1, 1)], 1)
            logits, nxt = step(nxt.view(1, 1).int())
    e, e32 = _logit_errors(logits, deq, seq)
    assert e <= max(4 * e32, 1e-5), (e, e32)
    assert state["pos"].tolist() == [11]


def test_mxfp4_prefill_over_eight_rows_takes_the_h3_path_and_matches(model, deq):
    """A 16-token prefill: every linear_mx4 but the one-row head dequantizes into a transient."""
    (pre, _), state = _compiled(model, "mxfp4", prompt_len=16)
    prompt = torch.randint(0, model.config.vocab_size, (1, 16), device="cuda")
    with torch.no_grad():
        logits, _ = pre(prompt.int())
    e, e32 = _logit_errors(logits, deq, prompt)
    assert e <= max(4 * e32, 1e-5), (e, e32)
    assert state["pos"].tolist() == [16]


def test_mxfp4_decode_step_keeps_every_fusion_of_the_fp32_step(model):
    (_, mx), _ = _compiled(model, "mxfp4")
    (_, f32), _ = _compiled(model, "fp32")
    layers = model.config.num_hidden_layers
    assert f32.stats["rmsnorm_folded"] == 2 * layers + 1     # the decode step's linears behind a norm
    assert mx.stats["mx4_rms_prologue"] == f32.stats["rmsnorm_folded"]
    assert mx.stats["mx4_glu_fused"] == f32.stats["gemv_glu_fused"] == layers
    assert mx.stats["mx4_combines_into_gemv"] == f32.stats["decode_combines_into_gemv"] == layers
    assert mx.stats["mx4_linears"] == 4 * layers + 1 and mx.stats["q8_linears"] == 0
    assert mx.stats["kernels"] <= f32.stats["kernels"]
    kinds = [s.kind for s in mx.steps]
    assert "linear" not in kinds and "glu" not in kinds and "rmsnorm" not in kinds and "linear_rms" not in kinds
    assert all(t.dtype != torch.float32 or t.dim() != 2 or k.startswith(("rope.", "model.embed"))
               for k, t in mx.consts.items()), "no fp32 copy of a quantized weight"


PROMPT_LEN, NEW, MAX_LEN = 16, 32, 64


def _prompt():   # seed 2: the fp64 reference's top-2 gap clears 1e-4 at every step (asserted where it is used)
    return np.random.default_rng(2).integers(0, 512, (1, PROMPT_LEN)).astype(np.int32)


def _greedy_fp64(m, **cache):
    """Greedy ids of ``m`` in fp64 and the smallest top-2 gap of its steps, relative to max |logit|."""
    m64 = copy.deepcopy(m).double()
    seq = torch.from_numpy(_prompt().astype(np.int64))
    gap = float("inf")
    with torch.no_grad():
        for _ in range(NEW):
            kw = {k: make() for k, make in cache.items()}
            logits = m64(seq, **kw).logits[0, -1]
            top = logits.topk(2)
            gap = min(gap, float((top.values[0] - top.values[1]) / logits.abs().max()))
            seq = torch.cat([seq, top.indices[:1].view(1, 1)], 1)
    return seq[:, PROMPT_LEN:].numpy(), gap


@pytest.fixture(scope="module")
def gpu_server(tmp_path_factory):
    from nos_amd.podserver.server import PodServer

    srv = PodServer(tmp_path_factory.mktemp("mx4") / "g.sock", device="cuda", lanes=2, memory_gb=40).start()
    yield srv
    srv.stop()


def _client(srv, tenant, name):
    from nos_amd.podserver.client import PodClient

    c = PodClient(srv.path, connect_timeout_s=60)
    c.register(name, tenant[0][0], tenant[1], memory_limit_gb=4, variants=tenant[0][1:])
    return c


@pytest.fixture(scope="module")
def plain_tokens(model, deq, gpu_server):
    """The plain MXFP4 tenant's tokens on the GPU server: the dequantized model's (asserted)."""
    from nos_amd.models.llama_program import llama_decode_programs

    want, gap = _greedy_fp64(deq)
    assert gap >= 1e-4, gap
    hf = deq.generate(torch.from_numpy(_prompt().astype(np.int64)), max_new_tokens=NEW, min_new_tokens=NEW,
                      do_sample=False, pad_token_id=0)[:, PROMPT_LEN:].numpy()
    assert np.array_equal(hf, want)
    c = _client(gpu_server, llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="mxfp4"), "llm-mx4")
    ids, tm = c.generate(_prompt(), NEW, server_loop=True)
    assert np.array_equal(ids, want), (ids, want)
    assert tm["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
    c.reset()
    again, tm2 = c.generate(_prompt(), NEW, server_loop=True)
    assert np.array_equal(again, want) and tm2["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
    c.close()
    return ids


def test_gpu_server_generates_the_dequantized_models_tokens(plain_tokens):
    """HIP graphs and the server loop; a second sequence after reset() repeats the first."""
    assert plain_tokens.shape == (1, NEW)


def test_gpu_server_mxfp4_with_int8_caches(model, deq, gpu_server):
    """``kv="int8"`` beside MXFP4 weights: the tokens of the dequantized model run with
    ``kv_q8_roundtrip_cache()`` (its fp64 top-2 gap asserted)."""
    from nos_amd.models.llama_program import kv_q8_roundtrip_cache, llama_decode_programs

    want, gap = _greedy_fp64(deq, past_key_values=kv_q8_roundtrip_cache)
    assert gap >= 1e-4, gap
    c = _client(gpu_server, llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="mxfp4", kv="int8"), "llm-mx4-kvq8")
    ids, _ = c.generate(_prompt(), NEW, server_loop=True)
    c.close()
    assert np.array_equal(ids, want), (ids, want)


def test_gpu_server_mxfp4_speculating_emits_the_plain_tenants_tokens(model, plain_tokens, gpu_server):
    from nos_amd.models.llama_program import llama_decode_programs

    c = _client(gpu_server, llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="mxfp4", speculate=4), "llm-mx4-spec")
    ids, t = c.generate(_prompt(), NEW, speculate=True)
    c.close()
    assert np.array_equal(ids, plain_tokens), (ids.tolist(), plain_tokens.tolist())
    assert t["state"] == {"pos": [PROMPT_LEN + NEW - 1]} and t["n_acc"].sum(0).tolist() == [NEW - 1]
