"""Multi-adapter LoRA on gfx950 (csrc/hip/decode.hip ``lora_shrink_kernel`` and
the adapter epilogue of ``gemv_kernel`` / ``gemv_q8_kernel``): the kernels
against fp64 at the project's bar (4x torch-fp32's own error, at least 2e-6
of max |y|; model logits: at least 1e-5), base rows bit for bit against the
plain kernels, then the compiled adapter tenant and the GPU pod server against
``adapted_llama``."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402
from nos_amd.ops import _lib, _stream  # noqa: E402
from nos_amd.ops import tenant as T  # noqa: E402
from test_lora import (MAX_LEN, NEW, PROMPT_LEN, adapters, make_adapters, model, prompt,  # noqa: E402, F401
                       reference)

N_AD = 3   # adapters n of the kernel tests


@pytest.fixture(autouse=True)
def _h3():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)


def _sel(M: int, rps: int, zero: bool = False) -> torch.Tensor:
    """An id per sequence of M rows: 0, valid ids, n + 1 and -1 mixed (row 0's is valid for M = 1)."""
    pat = [2, 0, N_AD + 1, 1, -1, 3, 0, 2] if M // rps > 1 or rps > 1 else [2]
    n = -(-M // rps)
    return torch.tensor([0] * n if zero else pat[:n], dtype=torch.int32, device="cuda")


def _valid_rows(sel: torch.Tensor, M: int, rps: int) -> torch.Tensor:
    a = sel.long().repeat_interleave(rps)[:M]
    return (a >= 1) & (a <= N_AD)


def _close(got, ref64, ref32, what, floor=2e-6) -> None:
    scale = float(ref64.abs().max()) or 1.0
    e = float((got.double() - ref64).abs().max()) / scale
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    print(f"{what}: e = {e:.3g}, e32 = {e32:.3g}")
    assert got.shape == ref64.shape and e <= max(4 * e32, floor), (what, e, e32)


def _adapter_weights(R: int, K: int, N: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(N_AD, R, K, generator=g) / K ** 0.5
    B = torch.randn(N_AD, N, R, generator=g) / R ** 0.5
    return A.cuda(), B.cuda()


# ------------------------------------------------------------------ 1. the shrink
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("K", [16, 256, 1040, 2816])
def test_lora_shrink_matches_fp64(M, K):
    """K below one 256-column step, a K tail, the down projection's K; every rank's wave layout; one
    and four rows per sequence; the RMSNorm prologue with and without gamma; strided x rows."""
    if M * K * 4 > 65536:
        M = 5   # 8 rows of 2816 are over the GEMV's 64 KiB of x (refused: the argument test)
    torch.manual_seed(M + K)
    xs = torch.randn(M, 2 * K, device="cuda")
    gamma = 1 + 0.1 * torch.randn(K, device="cuda")
    for R in (4, 12, 64):
        A, _ = _adapter_weights(R, K, 8, R + K)
        for rps in (1, 4):
            sel = _sel(M, rps)
            ok = _valid_rows(sel, M, rps)
            for x in (xs[:, :K].contiguous(), xs[:, K // 2:K // 2 + K] if (K // 2) % 4 == 0 else xs[:, :K]):
                for kw in ({}, {"rms_eps": 1e-5}, {"rms_eps": 1e-5, "gamma": gamma}):
                    got = T.lora_shrink(x, A, sel, rows_per_seq=rps, **kw)
                    assert got.shape == (M, R) and got.dtype == torch.float32
                    assert bool((got[~ok] == 0).all()), "a row without a valid adapter is exactly 0"
                    assert bool(ok.any()) and bool((got[ok] != 0).any())
                    _close(got, T.lora_shrink_ref(x, A, sel, rps, dtype=torch.float64, **kw),
                           T.lora_shrink_ref(x, A, sel, rps, dtype=torch.float32, **kw), (R, rps, tuple(kw)))


@pytest.mark.parametrize("D, B, G, Hkv", [(64, 1, 4, 2), (128, 2, 8, 1)])
def test_lora_shrink_combines_the_decode_partials(D, B, G, Hkv):
    """x given as the decode attention's split partials: combined as the O-projection's GEMV combines them."""
    L = 300
    torch.manual_seed(D + B + G + L)
    H = G * Hkv
    kc = torch.randn(B, L, Hkv, D, device="cuda")
    vc = torch.randn(B, L, Hkv, D, device="cuda")
    qq = torch.randn(B, 1, H, D, device="cuda")
    pos = torch.randint(0, L, (B,), dtype=torch.int32, device="cuda")
    pos[0] = L - 1
    A, Bw = _adapter_weights(12, H * D, 40, D)
    sel = torch.tensor([2, 0][:B], dtype=torch.int32, device="cuda")
    att = T.sdpa_cache(qq, kc, vc, pos).reshape(B, H * D)        # decode + attn_decode_combine
    p = T.sdpa_cache(qq, kc, vc, pos, partials=True)
    got = T.lora_shrink(p, A, sel)
    assert torch.equal(got, T.lora_shrink(att, A, sel))
    _close(got, T.lora_shrink_ref(att, A, sel, dtype=torch.float64), T.lora_shrink_ref(att, A, sel), "partials")
    # and the O-projection over the same partials with the adapter epilogue, fp32 and int8 weights
    w = torch.randn(40, H * D, device="cuda") / (H * D) ** 0.5
    res = torch.randn(B, 40, device="cuda")
    lora = (got, Bw, sel, 1)
    y = T.gemv_partials(p, w, None, None, res, lora=lora)
    assert torch.equal(y, T.gemv(att, w, None, None, res, lora=lora))
    q = torch.randint(-127, 128, (40, H * D), dtype=torch.int32).to(torch.int8).cuda()
    sc = (torch.rand(40) + 0.5).cuda() / (64.0 * (H * D) ** 0.5)
    y8 = T.gemv_q8_partials(p, q, sc, None, None, res, lora=lora)
    assert torch.equal(y8, T.gemv_q8(att, q, sc, None, None, res, lora=lora))
    if B > 1:   # sequence 1 runs the base model: the plain kernels' bits
        assert torch.equal(y[1], T.gemv_partials(p, w, None, None, res)[1])
        assert torch.equal(y8[1], T.gemv_q8_partials(p, q, sc, None, None, res)[1])


# ------------------------------------------------------------------ 2. the GEMVs with the adapter epilogue
def _gemv_cases(M, N, K, rps, seed):
    torch.manual_seed(seed)
    x = torch.randn(M, K, device="cuda")
    R = 12
    A, B = _adapter_weights(R, K, N, seed)
    sel = _sel(M, rps)
    b = torch.randn(N, device="cuda")
    r = torch.randn(M, N, device="cuda")
    return x, A, B, sel, b, r


def _run_epilogue_cases(M, N, K, run, ref, rms_kw):
    """``run(x, bias, act, res, lora=, **kw)`` against ``ref(..., dtype)``; base rows bit-equal to the plain call."""
    for rps in (1, 4):
        x, A, B, sel, b, r = _gemv_cases(M, N, K, rps, M + N + K + rps)
        ok = _valid_rows(sel, M, rps)
        zero = _sel(M, rps, zero=True)
        for kw in ({}, rms_kw):
            t = T.lora_shrink(x, A, sel, rows_per_seq=rps, **kw)
            t0 = T.lora_shrink(x, A, zero, rows_per_seq=rps, **kw)
            assert bool((t0 == 0).all())
            for act, bias, res in ((None, None, None), ("silu", b, None), (None, b, r), ("gelu", None, r)):
                plain = run(x, bias, act, res, **kw)
                got = run(x, bias, act, res, lora=(t, B, sel, rps), **kw)
                assert torch.equal(run(x, bias, act, res, lora=(t0, B, zero, rps), **kw), plain), "every sel = 0"
                assert torch.equal(got[~ok], plain[~ok]), "the sel = 0 (and out-of-range) rows of a mixed batch"
                assert bool(ok.any()) and not torch.equal(got[ok], plain[ok])
                args = (x, bias, act, res)
                _close(got, ref(*args, lora=(t, B, sel, rps), dtype=torch.float64, **kw),
                       ref(*args, lora=(t, B, sel, rps), dtype=torch.float32, **kw), (rps, act, tuple(kw)))


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("N, K", [(1, 16), (7, 256), (9, 1040), (1000, 256), (7, 2816)])
def test_gemv_with_the_adapter_epilogue_matches_fp64(M, N, K):
    if M * K * 4 > 65536:
        M = 5
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)).cuda() / K ** 0.5
    ones = torch.ones(N, device="cuda")

    def run(x, bias, act, res, lora=None, rms_eps=0.0):
        return T.gemv(x, w, bias, act, res, rms_eps=rms_eps, lora=lora)

    def ref(x, bias, act, res, lora, dtype, rms_eps=0.0):   # an fp32 W is its own dequantized weight
        return T.linear_q8_ref(x, w, ones, bias, act, res, rms_eps, None, False, dtype, lora=lora)

    _run_epilogue_cases(M, N, K, run, ref, {"rms_eps": 1e-5})


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("N, K", [(1, 16), (7, 256), (9, 1040), (1000, 256), (7, 2816)])
def test_gemv_q8_with_the_adapter_epilogue_matches_fp64(M, N, K):
    if M * K * 4 > 65536:
        M = 5
    g = torch.Generator().manual_seed(N + K)
    q = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int32).to(torch.int8).cuda()
    sc = ((torch.rand(N, generator=g) + 0.5) / (64.0 * K ** 0.5)).cuda()
    gamma = (1 + 0.1 * torch.randn(K, generator=g)).cuda()

    def run(x, bias, act, res, lora=None, **kw):
        return T.gemv_q8(x, q, sc, bias, act, res, lora=lora, **kw)

    def ref(x, bias, act, res, lora, dtype, **kw):
        return T.linear_q8_ref(x, q, sc, bias, act, res, dtype=dtype, lora=lora, **kw)

    _run_epilogue_cases(M, N, K, run, ref, {"rms_eps": 1e-5, "gamma": gamma})


@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("Nh, K", [(13, 64), (2816, 256)])
def test_glu_epilogue_takes_the_delta_on_gate_and_up(M, Nh, K):
    """The GLU form (W = [gate; up]): both products get their rows' delta; an odd half width."""
    g = torch.Generator().manual_seed(Nh + K)
    w = (torch.randn(2 * Nh, K, generator=g) / K ** 0.5).cuda()
    q = torch.randint(-127, 128, (2 * Nh, K), generator=g, dtype=torch.int32).to(torch.int8).cuda()
    sc = ((torch.rand(2 * Nh, generator=g) + 0.5) / (64.0 * K ** 0.5)).cuda()
    gamma = (1 + 0.1 * torch.randn(K, generator=g)).cuda()
    ones = torch.ones(2 * Nh, device="cuda")
    x, A, B, sel, _, _ = _gemv_cases(M, 2 * Nh, K, 1, Nh + M)
    ok = _valid_rows(sel, M, 1)
    for kw_g in ({}, {"rms_eps": 1e-5, "gamma": gamma}):
        t = T.lora_shrink(x, A, sel, **kw_g)
        lora = (t, B, sel, 1)
        got8 = T.gemv_q8(x, q, sc, glu=True, lora=lora, **kw_g)
        assert got8.shape == (M, Nh)
        assert torch.equal(got8[~ok], T.gemv_q8(x, q, sc, glu=True, **kw_g)[~ok])
        _close(got8, T.linear_q8_ref(x, q, sc, glu=True, dtype=torch.float64, lora=lora, **kw_g),
               T.linear_q8_ref(x, q, sc, glu=True, lora=lora, **kw_g), ("q8 glu", tuple(kw_g)))
    for eps in (0.0, 1e-5):
        t = T.lora_shrink(x, A, sel, rms_eps=eps)
        lora = (t, B, sel, 1)
        got = T.gemv(x, w, glu=True, rms_eps=eps, lora=lora)
        assert torch.equal(got[~ok], T.gemv(x, w, glu=True, rms_eps=eps)[~ok])
        _close(got, T.linear_q8_ref(x, w, ones, None, None, None, eps, None, True, torch.float64, lora=lora),
               T.linear_q8_ref(x, w, ones, None, None, None, eps, None, True, torch.float32, lora=lora), ("glu", eps))


# ------------------------------------------------------------------ 3. refusals
@pytest.mark.parametrize("case", ["null-t", "rank-6", "rank-68", "misaligned-a", "misaligned-b", "x-over-64k",
                                  "no-adapters", "short-b-stride"])
def test_bad_arguments_are_refused_without_a_launch(case):
    M, N, K, R = (8, 16, 2816, 8) if case == "x-over-64k" else (2, 16, 64, 8)
    if case == "rank-6":
        R = 6
    if case == "rank-68":
        R = 68
    x = torch.randn(M, K, device="cuda")
    store = torch.ones(N_AD * max(R, N) * max(K, R) + 8, device="cuda")
    oa = 1 if case == "misaligned-a" else 0
    ob = 1 if case == "misaligned-b" else 0
    A = store[oa:oa + N_AD * R * K].view(N_AD, R, K)
    B = store[ob:ob + N_AD * N * R].view(N_AD, N, R)
    sel = torch.ones(M, dtype=torch.int32, device="cuda")
    t = torch.full((M, R), 7.0, device="cuda")
    y = torch.full((M, N), 7.0, device="cuda")
    w = torch.ones(N, K, device="cuda")
    q = torch.ones(N, K, dtype=torch.int8, device="cuda")
    sc = torch.ones(N, device="cuda")
    n = 0 if case == "no-adapters" else N_AD
    bsb = N * R - 1 if case == "short-b-stride" else N * R
    lib = _lib.lib()
    bad = 1   # hipErrorInvalidValue
    tp = None if case == "null-t" else t.data_ptr()
    parts = (None, 0, 0, 0, 0, 0)
    if case not in ("misaligned-b", "short-b-stride"):   # the shrink has no B
        rc = lib.nos_lora_shrink(x.data_ptr(), K, *parts, A.data_ptr(), R * K, K, sel.data_ptr(), n, 1, None, 0.0, tp,
                                 M, R, K, _stream())
        assert rc == bad, (case, rc)
    if case != "misaligned-a":                            # the GEMVs have no A
        rc = lib.nos_gemv_lora(x.data_ptr(), K, *parts, w.data_ptr(), K, None, None, 0, y.data_ptr(), N, M, N, K, 0, 0.0,
                               tp, B.data_ptr(), bsb, R, sel.data_ptr(), R, n, 1, _stream())
        assert rc == bad, (case, rc)
        rc = lib.nos_gemv_q8_lora(x.data_ptr(), K, *parts, q.data_ptr(), K, sc.data_ptr(), None, None, None, 0,
                                  y.data_ptr(), N, M, N, K, 0, 0.0, tp, B.data_ptr(), bsb, R, sel.data_ptr(), R, n, 1,
                                  _stream())
        assert rc == bad, (case, rc)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((t == 7.0).all())


def test_wrappers_refuse_rows_the_gemvs_do_not_take():
    """No quiet fall-back: nine rows with an adapter operand are an error, not a PyTorch product."""
    x = torch.randn(9, 64, device="cuda")
    A, B = _adapter_weights(8, 64, 16, 0)
    sel = torch.ones(9, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="lora_shrink"):
        T.lora_shrink(x, A, sel)
    t = torch.zeros(9, 8, device="cuda")
    q, sc = torch.ones(16, 64, dtype=torch.int8, device="cuda"), torch.ones(16, device="cuda")
    with pytest.raises(ValueError, match="adapter epilogue exists on the int8 GEMV only"):
        T.linear_q8(x, q, sc, lora=(t, B, sel, 1))
    with pytest.raises(ValueError, match="gemv_ok"):
        T.linear_lora(x, torch.ones(16, 64, device="cuda"), lora=(t, B, sel, 1))


# ------------------------------------------------------------------ 4. whole tenants
def _compiled(model, weights: str, ads, prompt_len: int = 8, max_len: int = 128, batch: int = 1):
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    progs, w = llama_decode_programs(model, prompt_len, max_len, batch=batch, weights=weights, adapters=ads)
    ps = PG.parse_variants(progs, w, gpu=True)
    params = ps[0].tensors("cuda")
    state = ps[0].state_tensors("cuda")
    return [p.compile("cuda", params=params, state=state) for p in ps], state


def _model_for(model, ads, a: int, weights: str):
    from nos_amd.models.llama_program import adapted_llama, dequantized_llama

    base = dequantized_llama(model) if weights == "int8" else model
    return copy.deepcopy(base if a == 0 else adapted_llama(base, ads[a - 1])).cuda()


def _logits_close(logits, m, seq, what) -> None:
    with torch.no_grad():
        f32 = m(seq).logits[:, -1:]
        ref64 = m.double()(seq).logits[:, -1:]
    _close(logits, ref64, f32, what, floor=1e-5)


@pytest.mark.parametrize("weights", ["fp32", "int8"])
def test_adapted_decode_step_logits_match_adapted_llama_in_fp64(model, adapters, weights):
    """Prefill 8 (8 rows of one sequence: the GEMVs, rows_per_seq 8) + 3 decode steps, adapters 2 and 0."""
    (pre, step), state = _compiled(model, weights, adapters)
    for a in (2, 0):
        state["adapter"].fill_(a)
        ids = torch.randint(0, model.config.vocab_size, (1, 8), device="cuda", generator=torch.Generator("cuda").manual_seed(a))
        seq = ids.clone()
        with torch.no_grad():
            logits, nxt = pre(ids.int())
            for _ in range(3):
                seq = torch.cat([seq, nxt.long().view(1, 1)], 1)
                logits, nxt = step(nxt.view(1, 1).int())
        _logits_close(logits, _model_for(model, adapters, a, weights), seq, (weights, a))
        assert state["pos"].tolist() == [11]


@pytest.mark.parametrize("weights", ["fp32", "int8"])
def test_adapted_decode_step_costs_one_launch_per_adapted_activation(model, adapters, weights):
    layers = model.config.num_hidden_layers
    (_, plain), _ = _compiled(model, weights, None)
    for ads, per_layer in ((adapters, 2), (make_adapters(model, 2, ("self_attn.q_proj", "self_attn.k_proj",
                                                                    "self_attn.v_proj", "self_attn.o_proj",
                                                                    "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"),
                                                         rank=4), 4)):
        (_, step), _ = _compiled(model, weights, ads)
        assert step.stats["lora_shrinks"] == step.stats["lora_fused"] == layers * per_layer
        assert step.stats["kernels"] == plain.stats["kernels"] + step.stats["lora_shrinks"]
        kinds = [s.kind for s in step.steps]
        assert "lora" not in kinds and "add" not in kinds and "rmsnorm" not in kinds and "glu" not in kinds
        assert sum(1 for s in step.steps if s.attrs.get("lora")) == layers * per_layer
        for k in ("q8_rms_prologue", "q8_glu_fused", "q8_combines_into_gemv", "rmsnorm_folded", "gemv_glu_fused",
                  "decode_combines_into_gemv", "kv_writes_into_attention", "pos_add_into_argmax", "residual_fused"):
            assert step.stats.get(k) == plain.stats.get(k), (k, step.stats.get(k), plain.stats.get(k))


def test_all_seven_projections_match_adapted_llama(model):
    ads = make_adapters(model, 2, ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
                                   "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"), rank=4)
    for weights in ("fp32", "int8"):
        (pre, step), state = _compiled(model, weights, ads)
        state["adapter"].fill_(1)
        ids = torch.randint(0, model.config.vocab_size, (1, 8), device="cuda")
        seq = ids.clone()
        with torch.no_grad():
            logits, nxt = pre(ids.int())
            for _ in range(2):
                seq = torch.cat([seq, nxt.long().view(1, 1)], 1)
                logits, nxt = step(nxt.view(1, 1).int())
        _logits_close(logits, _model_for(model, ads, 1, weights), seq, weights)


def test_prefill_over_eight_rows_with_mixed_adapters_matches(model, adapters):
    """batch 2 x 16 tokens: the lora nodes run as PyTorch ops on the device, sel read there."""
    (pre, _), state = _compiled(model, "fp32", adapters, prompt_len=16, batch=2)
    assert any(s.kind == "lora" for s in pre.steps) and pre.stats["lora_shrinks"] == 0
    ids = torch.randint(0, model.config.vocab_size, (2, 16), device="cuda")
    for pair in ([2, 0], [1, 3]):
        state["adapter"].copy_(torch.tensor(pair, dtype=torch.int32))
        with torch.no_grad():
            logits, _ = pre(ids.int())
        for row, a in enumerate(pair):
            _logits_close(logits[row:row + 1], _model_for(model, adapters, a, "fp32"), ids[row:row + 1], (pair, row))
        assert state["pos"].tolist() == [16, 16]


def test_rows_past_the_gemvs_x_staging_keep_the_lora_step():
    """8 rows of K = 2816 are 88 KiB of x, over the GEMVs' 64 KiB: that linear runs on the GEMM, which has
    no adapter epilogue, so the compiler leaves the lora node (5 rows fit and fuse)."""
    from nos_amd.podserver import program as PG
    from nos_amd.podserver.program import Builder

    for rows, fused in ((8, 0), (5, 1)):
        rng = np.random.default_rng(rows)
        b = Builder("wide")
        x = b.input("x", [1, rows, 2816], "fp32")
        sel = b.adapter_state(1)
        w = b.param("w", rng.standard_normal((64, 2816)) / 53.0)
        A = b.param("A", rng.standard_normal((N_AD, 8, 2816)) / 53.0)
        B = b.param("B", rng.standard_normal((N_AD, 64, 8)))
        prog, payload = b.build([b.op("add", b.op("linear", x, w), b.op("lora", x, A, B, sel), out="y")])
        p = PG.parse(prog, payload, gpu=True)
        c = p.compile("cuda")
        assert c.stats["lora_shrinks"] == c.stats["lora_fused"] == fused
        c.state["adapter"].fill_(2)
        xv = torch.randn(1, rows, 2816, device="cuda")
        got, = c(xv)
        ps = {k: v.double().cpu() for k, v in p.tensors("cpu").items()}
        sel_t = torch.tensor([2], dtype=torch.int32)
        ref64 = torch.nn.functional.linear(xv.double().cpu(), ps["w"]) + T.lora_ref(xv.double().cpu(), ps["A"], ps["B"], sel_t)
        ref32 = torch.nn.functional.linear(xv.cpu(), ps["w"].float()) + T.lora_ref(xv.cpu(), ps["A"].float(), ps["B"].float(),
                                                                                   sel_t)
        _close(got.cpu(), ref64, ref32, rows)


def test_gpu_server_generates_each_adapters_tokens(model, adapters, reference, tmp_path):
    """HIP graphs and the server loop: one captured graph serves every adapter and every mix."""
    from nos_amd.models.llama_program import adapted_llama, dequantized_llama, llama_decode_programs
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer
    from test_lora import greedy_ids_and_gap

    srv = PodServer(tmp_path / "g.sock", device="cuda", lanes=2, memory_gb=40).start()
    try:
        progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, adapters=adapters)
        c = PodClient(srv.path, connect_timeout_s=60)
        c.register("lora", progs[0], w, memory_limit_gb=4, variants=progs[1:])
        for a in (0, 1, 2, 3, 0):
            ids, tm = c.generate(prompt(), NEW, server_loop=True, adapter=a)
            assert np.array_equal(ids, reference[a]), (a, ids, reference[a])
            assert tm["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
        c.close()
        progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, batch=2, adapters=adapters)
        c = PodClient(srv.path, connect_timeout_s=60)
        c.register("lora-b2", progs[0], w, memory_limit_gb=4, variants=progs[1:])
        two = np.repeat(prompt(), 2, axis=0)
        for pair in ([2, 0], [1, 3]):
            c.reset()
            got, _ = c.generate(two, NEW, server_loop=True, adapter=pair)
            assert np.array_equal(got[0:1], reference[pair[0]]) and np.array_equal(got[1:2], reference[pair[1]]), pair
        c.close()
        want, gap = greedy_ids_and_gap(adapted_llama(dequantized_llama(model), adapters[1]), prompt())
        assert gap >= 1e-4, gap
        progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="int8", adapters=adapters)
        c = PodClient(srv.path, connect_timeout_s=60)
        c.register("lora-q8", progs[0], w, memory_limit_gb=4, variants=progs[1:])
        assert np.array_equal(c.generate(prompt(), NEW, server_loop=True, adapter=2)[0], want)
        c.close()
        # a verify step's K rows belong to one sequence (rows_per_seq = K): the same tokens in fewer steps
        progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, speculate=4, adapters=adapters)
        c = PodClient(srv.path, connect_timeout_s=60)
        c.register("lora-spec", progs[0], w, memory_limit_gb=4, variants=progs[1:])
        for a in (3, 0):
            spec, _ = c.generate(prompt(), NEW, adapter=a, speculate=True)
            assert np.array_equal(spec, reference[a]), a
        c.close()
    finally:
        srv.stop()
