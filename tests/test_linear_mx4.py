"""MXFP4 weight-only decoder tenants (CPU): the block quantizer against an
independent fp64 formulation, the ``u8`` wire dtype and the ``linear_mx4`` op
through validator, eager reference, Llama builder, accounting and the CPU pod
server.  Quantization is a storage format: everything is compared against the
dequantized weights (``dequantized_llama(model, "mxfp4")``), never against the
fp32 model."""
from __future__ import annotations

import copy
import json
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nos_amd.models.llama_program import (dequantized_llama, kv_q8_roundtrip_cache, llama_config,
                                          llama_decode_programs, llama_model, mixtral_config, mixtral_model)
from nos_amd.ops import tenant as T
from nos_amd.podserver import program as PG
from nos_amd.podserver.client import PodClient, PodServerError
from nos_amd.podserver.program import Builder, ProgramError, dequantize_rows_mx4, ir, quantize_rows_mx4
from nos_amd.podserver.server import PodServer

PROMPT_LEN, NEW, MAX_LEN = 16, 32, 64
PROMPT_SEED = 2   # re-checked for MXFP4 weights: the dequantized fp64 reference's top-2 gap clears 1e-4 (asserted below)
GRID = [Fraction(v) for v in (0, 0.5, 1, 1.5, 2, 3, 4, 6)]


@pytest.fixture(scope="module")
def model():
    return llama_model(llama_config(False), 0)


@pytest.fixture(scope="module")
def deq(model):
    return dequantized_llama(model, weights="mxfp4")


@pytest.fixture(scope="module")
def tenant_mx4(model):
    return llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="mxfp4")


@pytest.fixture(scope="module")
def tenant_f32(model):
    return llama_decode_programs(model, PROMPT_LEN, MAX_LEN)


# ------------------------------------------------------------------ 1. the quantizer
def _quantize_block_exact(block: np.ndarray) -> tuple[list[int], int]:
    """One block of 32 in exact rational arithmetic, written from the format's words alone: the scale
    exponent by repeated doubling / halving, each element to the nearest grid value by distance, a tie
    to the even code."""
    vals = [Fraction(float(v)) for v in block]
    amax = max(abs(v) for v in vals)
    if amax == 0:
        e = 127
    else:
        p = 0                                   # floor(log2(amax)): 2^p <= amax < 2^(p + 1)
        while Fraction(2) ** (p + 1) <= amax:
            p += 1
        while Fraction(2) ** p > amax:
            p -= 1
        e = min(max(p - 2 + 127, 2), 252)
    scale = Fraction(2) ** (e - 127)
    codes = []
    for v, raw in zip(vals, block):
        a = abs(v) / scale
        best = min(range(8), key=lambda c: (abs(GRID[c] - a), c % 2))   # nearest; of two equally near, the even code
        codes.append(best | (8 if np.signbit(raw) else 0))
    return codes, e


def _check_against_exact(w: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    codes, scales = quantize_rows_mx4(w)
    N, K = w.shape
    assert codes.dtype == np.uint8 and codes.shape == (N, K // 2) and scales.dtype == np.uint8 and scales.shape == (N, K // 32)
    for n in range(N):
        for b in range(K // 32):
            want, e = _quantize_block_exact(w[n, 32 * b:32 * b + 32])
            got = [int(codes[n, 16 * b + i // 2] >> (4 * (i % 2))) & 15 for i in range(32)]
            assert int(scales[n, b]) == e and got == want, (n, b, e, int(scales[n, b]))
    return codes, scales


def test_quantizer_matches_the_exact_formulation_on_gaussian_rows_and_reaches_every_code():
    rng = np.random.default_rng(0)
    w = (rng.standard_normal((6, 96)) * rng.uniform(1e-3, 30, (6, 1))).astype(np.float32)
    w[2, 32:64] = 0.0                                          # an all-zero block
    codes, scales = _check_against_exact(w)
    assert scales[2, 1] == 127 and not codes[2, 16:32].any()
    assert set((codes & 15).ravel().tolist()) | set((codes >> 4).ravel().tolist()) == set(range(16))
    assert 2 <= scales.min() and scales.max() <= 252
    back = dequantize_rows_mx4(codes, scales)
    assert back.dtype == np.float32 and back.shape == w.shape
    # within a block the error is at most half the widest grid step (1 between 4 and 6 ... times the scale),
    # except where the value saturates: |v| in (6, 8) scale clamps to 6 scale
    s = np.repeat(np.ldexp(1.0, scales.astype(np.int32) - 127), 32, axis=1)
    assert np.all(np.abs(back.astype(np.float64) - w) <= 2.0 * s + 1e-30)
    sat = np.abs(w) > 6 * s
    assert sat.any() and np.all(np.abs(back[sat]) == 6 * s[sat])


def test_quantizer_ties_go_to_the_even_code_and_values_saturate():
    for sh in (-3, 0, 5):                                      # the scale 2^sh: the block maximum 4 .. 8 times it
        s = 2.0 ** sh
        ties = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}
        v = np.zeros((1, 32), np.float32)
        v[0, 0] = 4.0 * s                                      # fixes the block's scale at 2^sh, itself exact
        for i, t in enumerate(ties):
            v[0, 1 + i], v[0, 9 + i] = t * s, -t * s
        v[0, 17:22] = np.array([6.0, 6.5, 7.0, 7.999, -7.5], np.float32) * s      # (6, 8) x scale saturates at 6
        codes, scales = _check_against_exact(v)
        assert int(scales[0, 0]) == 127 + sh
        back = dequantize_rows_mx4(codes, scales)[0] / s
        assert back[1:8].tolist() == list(ties.values()) and back[9:16].tolist() == [-t for t in ties.values()]
        assert back[17:22].tolist() == [6.0, 6.0, 6.0, 6.0, -6.0] and back[0] == 4.0


def test_quantizer_clamps_the_scale_at_both_ends_to_normal_finite_values():
    sub = np.full((1, 32), np.float32(1e-40))                  # fp32 subnormals: e clamps at 2, the elements round to 0
    sub[0, 5] = -np.float32(3e-39)
    codes, scales = _check_against_exact(sub)
    assert scales.tolist() == [[2]] and set((codes & 7).ravel().tolist()) | set(((codes >> 4) & 7).ravel().tolist()) == {0}
    near = np.zeros((1, 32), np.float32)
    near[0, :4] = [2.0 ** -126, -(2.0 ** -125), 0.6 * 2.0 ** -126, 0.4 * 2.0 ** -126]   # the smallest kept: 0.5 x 2^-125
    back = dequantize_rows_mx4(*_check_against_exact(near))
    assert back[0, :4].tolist() == [2.0 ** -126, -(2.0 ** -125), 2.0 ** -126, 0.0] and np.all(np.abs(back[back != 0]) >= np.finfo(np.float32).tiny)
    big = np.full((1, 32), np.float32(3e38))
    big[0, 1] = -np.float32(1e38)
    codes, scales = _check_against_exact(big)
    back = dequantize_rows_mx4(codes, scales)
    assert scales.tolist() == [[252]] and np.isfinite(back).all() and back[0, 0] == 6 * 2.0 ** 125
    assert 255 not in scales and back.dtype == np.float32


def test_quantizer_is_idempotent_in_value_and_packs_low_nibble_first():
    rng = np.random.default_rng(1)
    w = (rng.standard_normal((16, 128)) * 0.02).astype(np.float32)
    w[3, :32] = 1e-42
    w[4, 32:64] = 3e38
    w[5, 64:96] *= 1e-3 * (rng.random(32) < 0.1)               # a block most of which rounds to zero
    d1 = dequantize_rows_mx4(*quantize_rows_mx4(w))
    d2 = dequantize_rows_mx4(*quantize_rows_mx4(d1))
    assert np.array_equal(d1.view(np.int32), d2.view(np.int32))
    v = np.zeros((1, 32), np.float32)
    v[0, :4] = [4.0, 0.5, -1.5, 3.0]                            # codes 6, 1, 0xb, 5
    codes, _ = quantize_rows_mx4(v)
    assert codes[0, :2].tolist() == [0x16, 0x5b] and not codes[0, 2:].any()
    assert dequantize_rows_mx4(np.array([[0x80] + [0] * 15], np.uint8), np.array([[127]], np.uint8))[0, :2].tolist() == [0.0, -0.0]
    frac = float((np.abs(w[6:]) > 6 * np.repeat(np.ldexp(1.0, quantize_rows_mx4(w[6:])[1].astype(np.int32) - 127), 32, 1)).mean())
    assert 0.0 < frac < 0.06, frac                              # a few per cent of Gaussian elements saturate: the format


@pytest.mark.parametrize("shape", [(4, 48), (4, 31), (64,)])
def test_quantizer_refuses_k_that_is_no_multiple_of_32(shape):
    with pytest.raises(ValueError, match="K % 32"):
        quantize_rows_mx4(np.ones(shape, np.float32))
    with pytest.raises(ValueError, match="K / 32"):
        dequantize_rows_mx4(np.zeros((2, 16), np.uint8), np.zeros((2, 2), np.uint8))


# ------------------------------------------------------------------ 2. the validator
def _mx4_program(k: int = 64, n: int = 24, x_dtype: str = "fp32", bias: bool = True, w=None):
    rng = np.random.default_rng(1)
    b = Builder("mx4")
    x = b.input("x", [3, k], "fp32")
    if x_dtype != "fp32":
        x = b.op("cast", x, dtype=x_dtype)
    wq, sc = b.param_mx4("w", rng.standard_normal((n, k)) if w is None else w)
    ins = [x, wq, sc] + ([b.param("bias", rng.standard_normal(n))] if bias else [])
    y = b.op("linear_mx4", *ins, act="gelu", out="y")
    return b.build([y])


def test_validator_accepts_a_well_formed_linear_mx4():
    prog, w = _mx4_program()
    p = PG.parse(prog, w, gpu=True)
    assert p.values["y"].shape == (3, 24) and p.values["y"].dtype == "fp32"
    assert p.params["w.mx4"].dtype == "u8" and p.params["w.mx4"].shape == (24, 32)
    assert p.params["w.e8m0"].dtype == "u8" and p.params["w.e8m0"].shape == (24, 2)
    assert p.param_bytes == 24 * 64 // 2 + 24 * 64 // 32 + 24 * 4
    t = p.tensors("cpu")
    assert t["w.mx4"].dtype == torch.uint8 and t["w.e8m0"].dtype == torch.uint8 and PG.torch_dtype("u8") == torch.uint8
    assert "linear_mx4" in PG.OPS and "linear_mx4" in PG.NATIVE_KINDS and "linear_mx4" in PG.NEVER_FOLD
    assert ir.WIRE_DTYPES["u8"] == 1 and "u8" in ir.PARAM_DTYPES and "u8" not in ir.STATE_DTYPES


def _mutated(mutate, **kw):
    prog, w = _mx4_program(**kw)
    prog = copy.deepcopy(prog)
    mutate(prog)
    return prog, w


def _node(prog, op):
    return next(n for n in prog["nodes"] if n["op"] == op)


def _param(prog, name):
    return next(q for q in prog["params"] if q["name"] == name)


def _use_in_linear(p):
    _node(p, "linear_mx4").update(op="linear", inputs=["x", "w.mx4"])


def _use_in_linear_q8(p):
    _node(p, "linear_mx4").update(op="linear_q8")


def _use_in_embedding(p):
    p["inputs"][0].update(dtype="i32")
    _node(p, "linear_mx4").update(op="embedding", inputs=["x", "w.e8m0"], attrs={})


def _codes_as_bias(p):
    n = _node(p, "linear_mx4")
    n["inputs"] = n["inputs"][:3] + ["w.e8m0"]


def _u8_as_x(p):
    n = _node(p, "linear_mx4")
    n["inputs"] = ["w.mx4"] + n["inputs"][1:]


def _wrong_scale_shape(p):
    _param(p, "w.e8m0").update(shape=[12, 4])


def _scale_not_u8(p):
    _node(p, "linear_mx4")["inputs"][2] = "bias"


@pytest.mark.parametrize("mutate, match", [
    (lambda p: p["inputs"][0].update(dtype="u8"), "input dtype u8"),
    (lambda p: p.update(state=[{"name": "s", "shape": [4], "dtype": "u8"}]), "state dtype u8"),
    (lambda p: p["outputs"].append("w.mx4"), "u8 param cannot be an output"),
    (lambda p: p["outputs"].append("w.e8m0"), "u8 param cannot be an output"),
    (_use_in_linear, "only linear_mx4 takes one"),
    (_use_in_linear_q8, "only linear_mx4 takes one"),
    (_use_in_embedding, "only linear_mx4 takes one"),
    (_codes_as_bias, "only linear_mx4 takes one"),
    (_u8_as_x, "only linear_mx4 takes one"),
    (_wrong_scale_shape, "wscale must be a u8"),
    (_scale_not_u8, "wscale must be a u8"),
    (lambda p: _param(p, "w.mx4").update(nbytes=24 * 64), "nbytes"),
], ids=["u8-input", "u8-state", "codes-output", "scales-output", "u8-in-linear", "u8-in-linear_q8", "u8-in-embedding",
        "u8-as-bias", "u8-as-x", "wscale-shape", "wscale-dtype", "nbytes"])
def test_validator_refusals(mutate, match):
    prog, w = _mutated(mutate)
    with pytest.raises(ProgramError, match=match):
        PG.parse(prog, w)


def test_validator_names_the_node_and_refuses_a_bf16_x_and_k_48():
    prog, w = _mutated(_use_in_linear)
    with pytest.raises(ProgramError, match=r"'y' \(linear\)"):
        PG.parse(prog, w)
    prog, w = _mx4_program(x_dtype="bf16")
    with pytest.raises(ProgramError, match="fp32"):
        PG.parse(prog, w)

    def k48(p):     # codes [24, 24] and scales [24, 1] of a K = 48 x: no whole number of blocks
        p["inputs"][0].update(shape=[3, 48])
        _param(p, "w.mx4").update(shape=[24, 24], nbytes=24 * 24)
        _param(p, "w.e8m0").update(shape=[24, 1], nbytes=24)
    prog, w = _mutated(k48)
    for gpu in (False, True):
        with pytest.raises(ProgramError, match="K % 32"):
            PG.parse(prog, w, gpu=gpu)


@pytest.mark.parametrize("byte", [0, 1, 253, 254, 255])
def test_a_scale_byte_outside_2_to_252_is_refused_when_the_payload_becomes_tensors(byte, tmp_path):
    prog, w = _mx4_program()
    off = _param(prog, "w.e8m0")["offset"]
    bad = bytearray(w)
    bad[off + 5] = byte
    p = PG.parse(prog, bytes(bad))                            # the wire format is well formed ...
    with pytest.raises(ValueError, match=rf"scale byte {byte} is outside \[2, 252\]"):
        p.tensors("cpu")                                      # ... and the registration's host pass refuses it
    for ok in (2, 252):
        bad[off + 5] = ok
        PG.parse(prog, bytes(bad)).tensors("cpu")
    if byte == 255:                                           # through a server: the registration fails, nothing is built
        bad[off + 5] = byte
        srv = PodServer(tmp_path / "s.sock", device="cpu", lanes=2, memory_gb=40).start()
        try:
            c = PodClient(srv.path, connect_timeout_s=5)
            with pytest.raises(PodServerError, match="scale byte 255"):
                c.register("bad", prog, bytes(bad), memory_limit_gb=1)
            c.close()
        finally:
            srv.stop()


# ------------------------------------------------------------------ 3. the eager reference
@pytest.mark.parametrize("bias", [False, True])
def test_reference_is_f_linear_on_the_dequantized_weight_bit_for_bit(bias):
    prog, w = _mx4_program(bias=bias)
    _node(prog, "linear_mx4")["attrs"] = {}
    p = PG.parse(prog, w)
    t = p.tensors("cpu")
    x = torch.randn(3, 64, generator=torch.Generator().manual_seed(2))
    wf = torch.from_numpy(dequantize_rows_mx4(t["w.mx4"].numpy(), t["w.e8m0"].numpy()))
    want = F.linear(x, wf, t["bias"] if bias else None)
    assert torch.equal(p.reference(x)[0], want)
    assert torch.equal(p.compile("cpu")(x)[0], want)
    assert torch.equal(T.linear_mx4(x, t["w.mx4"], t["w.e8m0"], t["bias"] if bias else None), want)
    assert torch.equal(T.dequant_mx4(t["w.mx4"], t["w.e8m0"]).view(torch.int32), wf.view(torch.int32))
    ref64 = T.linear_mx4_ref(x, t["w.mx4"], t["w.e8m0"], t["bias"] if bias else None, dtype=torch.float64)
    assert ref64.dtype == torch.float64 and float((ref64 - want.double()).abs().max()) < 1e-5
    gamma = torch.rand(64) + 0.5
    r = torch.randn(3, 12)
    y = T.linear_mx4_ref(x, t["w.mx4"], t["w.e8m0"], None, None, r, rms_eps=1e-5, gamma=gamma, glu=True)
    xn = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * gamma
    full = F.linear(xn, wf)
    assert torch.allclose(y, F.silu(full[:, :12]) * full[:, 12:] + r, rtol=1e-6, atol=1e-6)


def test_linear_mx4_is_never_folded_into_an_fp32_weight():
    """All of its inputs constant: still a step (folding would materialise the fp32 weight)."""
    b = Builder("const")
    x = b.input("x", [1, 64], "fp32")
    c = b.param("c", np.ones((2, 64), np.float32))
    wq, sc = b.param_mx4("w", np.random.default_rng(0).standard_normal((8, 64)))
    y = b.op("add", b.op("linear_mx4", c, wq, sc), b.op("slice", x, dim=-1, start=0, end=8))
    prog, w = b.build([y])
    p = PG.parse(prog, w)
    assert not p.foldable()
    cp = p.compile("cpu")
    assert cp.stats["constant_folded"] == 0 and cp.stats["mx4_linears"] == 1 and cp.stats["q8_linears"] == 0
    assert cp.consts["w.mx4"].dtype == torch.uint8 and not any(v.dtype == torch.float32 and v.shape == (8, 64)
                                                               for v in cp.consts.values())


# ------------------------------------------------------------------ 4. the Llama builder
def test_llama_mxfp4_programs_hold_codes_and_block_scales(model, tenant_mx4, tenant_f32):
    progs, w = tenant_mx4
    ps = PG.parse_variants(progs, w)
    assert [p.inputs[0].shape for p in ps] == [(1, PROMPT_LEN), (1, 1)]
    assert all("-mx4-" in p["name"] for p in progs)
    cfg = model.config
    codes = {k: v for k, v in ps[0].params.items() if k.endswith(".mx4")}
    assert len(codes) == 4 * cfg.num_hidden_layers + 1          # qkv, o, gate_up, down per layer + the head
    assert ps[0].params["model.embed_tokens.weight"].dtype == "fp32"
    assert not any(n.op in ("linear", "linear_q8") for p in ps for n in p.nodes)
    total = 0
    for name, v in codes.items():                              # per linear: N K / 2 bytes of codes, N K / 32 of scales
        sc = ps[0].params[name[:-4] + ".e8m0"]
        N, K = v.shape[0], v.shape[1] * 2
        assert v.dtype == sc.dtype == "u8" and v.nbytes == N * K // 2 and sc.shape == (N, K // 32) and sc.nbytes == N * K // 32
        total += N * K
    f32 = PG.parse_variants(*tenant_f32)
    assert f32[0].param_bytes - ps[0].param_bytes == 4 * total - total * 17 // 32
    assert len(w) < len(tenant_f32[1]) - 3.4 * total


def test_fp32_and_int8_programs_are_byte_identical_beside_an_mxfp4_build(model, tenant_f32):
    before = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="int8")
    llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="mxfp4")
    after = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="int8")
    assert before[1] == after[1] and json.dumps(before[0]) == json.dumps(after[0])
    again = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="fp32")
    assert again[1] == tenant_f32[1] and json.dumps(again[0]) == json.dumps(tenant_f32[0])
    assert not any(v["dtype"] == "u8" for t in (before, tenant_f32) for p in t[0] for v in p["params"])
    assert not any(n["op"] == "linear_mx4" for t in (before, tenant_f32) for p in t[0] for n in p["nodes"])
    assert [p["name"] for p in before[0]] == ["llama-h256-l2-fp32-q8-prefill16", "llama-h256-l2-fp32-q8-step1"]


def test_builder_refusals_each_name_their_rule(model):
    with pytest.raises(ValueError, match="dtype must be 'fp32'"):
        llama_decode_programs(model, PROMPT_LEN, MAX_LEN, dtype="bf16", weights="mxfp4")
    A = np.zeros((4, model.config.hidden_size), np.float32)
    B = np.zeros((model.config.hidden_size, 4), np.float32)
    with pytest.raises(ValueError, match="no adapter epilogue"):
        llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="mxfp4",
                              adapters=[{"model.layers.0.self_attn.o_proj": (A, B, 1.0)}])
    with pytest.raises(ValueError, match="no quantized experts"):
        llama_decode_programs(mixtral_model(mixtral_config(), 0), PROMPT_LEN, MAX_LEN, weights="mxfp4")
    for kw, what in (({"hidden_size": 144, "num_attention_heads": 3, "num_key_value_heads": 3}, "hidden_size = 144"),
                     ({"intermediate_size": 336}, "intermediate_size = 336")):
        m = llama_model(llama_config(False, num_hidden_layers=1, **kw), 0)
        with pytest.raises(ValueError, match=f"{what} is not a multiple of 32"):
            llama_decode_programs(m, 4, 16, weights="mxfp4")
    with pytest.raises(ValueError, match="weights"):
        llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="int4")
    with pytest.raises(ValueError, match="'int8' or 'mxfp4'"):
        dequantized_llama(model, weights="fp32")
    with pytest.raises(ValueError, match="MXFP4"):              # the int8 staging rule: batch * K * widest * 4 <= GEMV_X_BYTES
        big = llama_model(llama_config(False, num_hidden_layers=1, intermediate_size=4128), 0)
        llama_decode_programs(big, 5, 16, weights="mxfp4", speculate=4)


@pytest.mark.parametrize("kw", [
    {"batch": 2}, {"extend": (4,)}, {"sampling": True}, {"stopping": True}, {"kv": "int8"}, {"window": 24},
    {"speculate": 4}, {"batch": 2, "extend": (3,), "sampling": True, "stopping": True, "kv": "int8", "window": 24},
    {"speculate": 4, "kv": "int8", "window": 24},
], ids=lambda kw: "+".join(kw))
def test_the_combinations_build_and_validate(model, kw):
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="mxfp4", **kw)
    ps = PG.parse_variants(progs, w, gpu=True)
    assert len(ps) == 2 + len(kw.get("extend", ())) + ("speculate" in kw)
    assert all(any(n.op == "linear_mx4" for n in p.nodes) and not any(n.op in ("linear", "linear_q8") for n in p.nodes)
               for p in ps)


def test_a_tied_head_gets_its_own_quantized_copy():
    m = llama_model(llama_config(False, tie_word_embeddings=True, num_hidden_layers=1), 0)
    progs, w = llama_decode_programs(m, 4, 16, weights="mxfp4")
    p = PG.parse_variants(progs, w)[0]
    assert p.params["model.embed_tokens.weight"].dtype == "fp32" and p.params["lm_head.weight.mx4"].dtype == "u8"
    d = dequantized_llama(m, weights="mxfp4")
    assert torch.equal(d.model.embed_tokens.weight, m.model.embed_tokens.weight)
    assert not torch.equal(d.lm_head.weight, m.lm_head.weight)
    ids = torch.randint(0, 512, (1, 4), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = d(ids).logits[:, -1:]
    got = p.reference(ids.int())[0]
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_compiled_decode_step_keeps_the_rms_prologue_and_epilogues(tenant_mx4):
    ps = PG.parse_variants(*tenant_mx4)
    c = ps[1].compile("cpu", params=ps[0].tensors("cpu"))
    layers = sum(1 for n in ps[1].nodes if n.op == "sdpa_cache")
    assert c.stats["mx4_linears"] == 4 * layers + 1 and c.stats["mx4_rms_prologue"] == 2 * layers + 1
    assert c.stats["q8_linears"] == 0 and c.stats["q8_rms_prologue"] == 0
    assert c.stats["rmsnorm_folded"] == 0 and c.stats["linears_merged"] == 0
    assert c.stats["residual_fused"] == 2 * layers
    kinds = [s.kind for s in c.steps]
    assert "rmsnorm" not in kinds and "add" not in kinds and "linear" not in kinds
    assert all(v.dtype != torch.float32 or v.dim() != 2 or k.startswith(("rope.", "model.embed"))
               for k, v in c.consts.items()), "no fp32 copy of a quantized weight"


# ------------------------------------------------------------------ 5. reference and CPU server against the dequantized model
def _prompt() -> np.ndarray:
    return np.random.default_rng(PROMPT_SEED).integers(0, 512, (1, PROMPT_LEN)).astype(np.int32)


def reference_ids_and_gap(deq, new: int = NEW, **cache) -> tuple[np.ndarray, float]:
    """Greedy ids of the dequantized model in fp64, and the smallest top-2 logit gap over the generated
    steps relative to the largest |logit|.  ``cache``: name -> a factory of a fresh cache per step."""
    m64 = copy.deepcopy(deq).double()
    seq = torch.from_numpy(_prompt().astype(np.int64))
    gap = float("inf")
    with torch.no_grad():
        for _ in range(new):
            logits = m64(seq, **{k: make() for k, make in cache.items()}).logits[0, -1]
            top = logits.topk(2)
            gap = min(gap, float((top.values[0] - top.values[1]) / logits.abs().max()))
            seq = torch.cat([seq, top.indices[:1].view(1, 1)], 1)
    return seq[:, PROMPT_LEN:].numpy(), gap


@pytest.fixture(scope="module")
def reference(deq):
    want, gap = reference_ids_and_gap(deq)
    assert gap >= 1e-4, f"top-2 gap {gap}: pick another PROMPT_SEED (the test must not ride on a near tie)"
    return want


def test_eager_reference_logits_match_the_dequantized_model(deq, tenant_mx4):
    """Prefill, then three decode steps over one state: the last step's logits at the fp32 bar."""
    ps = PG.parse_variants(*tenant_mx4)
    params = ps[0].tensors("cpu")
    state = {k: (t if t.dtype in (torch.int32, torch.int8) else t.float()) for k, t in ps[0].state_tensors("cpu").items()}
    seq = torch.from_numpy(_prompt().astype(np.int64))
    logits, nxt = ps[0].reference(seq.int(), params, state)
    for _ in range(3):
        seq = torch.cat([seq, nxt.long().view(1, 1)], 1)
        logits, nxt = ps[1].reference(nxt.view(1, 1).int(), params, state)
    with torch.no_grad():
        f32 = deq(seq).logits[:, -1:]
        ref64 = copy.deepcopy(deq).double()(seq).logits[:, -1:]
    e = float((logits.double() - ref64).abs().max() / ref64.abs().max())
    e32 = float((f32.double() - ref64).abs().max() / ref64.abs().max())
    print(f"e = {e:.3g}, e32 = {e32:.3g}")
    assert e <= max(4 * e32, 1e-5), (e, e32)


@pytest.fixture(scope="module")
def cpu_server(tmp_path_factory):
    import shutil
    import tempfile
    from pathlib import Path

    d = Path(tempfile.mkdtemp(prefix="nos_mx4_"))
    srv = PodServer(d / "s.sock", device="cpu", lanes=2, memory_gb=40).start()
    yield srv
    srv.stop()
    shutil.rmtree(d, ignore_errors=True)


def _generate(srv, name, tenant, new=NEW, **kw):
    c = PodClient(srv.path, connect_timeout_s=5)
    try:
        c.register(name, tenant[0][0], tenant[1], memory_limit_gb=1, variants=tenant[0][1:])
        return c.generate(_prompt(), new, **kw)
    finally:
        c.close()


def test_cpu_server_generates_the_dequantized_models_tokens(deq, reference, tenant_mx4, cpu_server):
    hf = deq.generate(torch.from_numpy(_prompt().astype(np.int64)), max_new_tokens=NEW, min_new_tokens=NEW,
                      do_sample=False, pad_token_id=0)[:, PROMPT_LEN:].numpy()
    assert np.array_equal(hf, reference)
    a, ta = _generate(cpu_server, "mx4-loop", tenant_mx4, server_loop=True)
    b, tb = _generate(cpu_server, "mx4-steps", tenant_mx4, server_loop=False)
    assert np.array_equal(a, reference) and np.array_equal(b, reference)
    assert ta["state"] == tb["state"] == {"pos": [PROMPT_LEN + NEW - 1]}


def test_cpu_server_with_int8_caches(model, deq, cpu_server):
    want, gap = reference_ids_and_gap(deq, past_key_values=kv_q8_roundtrip_cache)
    assert gap >= 1e-4, gap
    ids, _ = _generate(cpu_server, "mx4-kvq8", llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="mxfp4", kv="int8"))
    assert np.array_equal(ids, want)


def test_cpu_server_with_a_window_below_max_len(model, deq, cpu_server):
    """A window of 24 < 64: the dequantized model as a Mistral with that ``sliding_window``."""
    from nos_amd.models.llama_program import mistral_config, mistral_model

    mis = mistral_model(mistral_config(sliding_window=24), 0)
    mis.load_state_dict(deq.state_dict())
    want, gap = reference_ids_and_gap(mis.eval())
    assert gap >= 1e-4, gap
    ids, _ = _generate(cpu_server, "mx4-swa", llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="mxfp4", window=24))
    assert np.array_equal(ids, want)


def test_cpu_server_stopping_ends_at_a_stop_id_like_the_dequantized_model(model, reference, cpu_server):
    stop = int(reference[0, 5])
    first = int(np.argmax(reference[0] == stop))
    tenant = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="mxfp4", stopping=True)
    ids, _ = _generate(cpu_server, "mx4-stop", tenant, eos_token_id=[stop], pad_token_id=0)
    ids = np.asarray(ids)
    assert np.array_equal(ids[0, :first + 1], reference[0, :first + 1])
    assert not ids[0, first + 1:].any()


# ------------------------------------------------------------------ 6. admission
def _need(progs, kernel_config) -> int:
    """The server's static estimate of a tenant's variants (the weights and the state once)."""
    return (sum(p.bytes_estimate_for(kernel_config) for p in progs)
            - (len(progs) - 1) * (progs[0].param_bytes + progs[0].state_bytes))


def test_static_estimate_charges_a_u8_param_one_byte_and_a_prefill_its_transient_weight(model, tenant_mx4, tenant_f32):
    pm, pf = PG.parse_variants(*tenant_mx4), PG.parse_variants(*tenant_f32)
    pq = PG.parse_variants(*llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="int8"))
    cfg = {"f32_math": "h3"}
    assert _need(pm, cfg) < _need(pq, cfg) < _need(pf, cfg)
    u8 = sum(v.numel for v in pm[1].params.values() if v.dtype == "u8")
    assert pm[1].param_bytes == u8 + sum(v.nbytes for v in pm[1].params.values() if v.dtype != "u8")
    # the quantized tenants differ by their params alone: no planes, no copies, the same activations and workspaces
    assert _need(pq, cfg) - _need(pm, cfg) == pq[0].param_bytes - pm[0].param_bytes
    lin = next(n for n in pm[1].nodes if n.op == "linear_mx4")
    ins = [pm[1].values[i] for i in lin.inputs]
    assert PG._workspace(lin, ins, pm[1].values[lin.output], "h3") == 0          # a decode step: the GEMV
    lin0 = next(n for n in pm[0].nodes if n.op == "linear_mx4")
    ins0 = [pm[0].values[i] for i in lin0.inputs]
    N, K, M = ins0[1].shape[0], ins0[0].shape[-1], PROMPT_LEN
    assert PG._workspace(lin0, ins0, pm[0].values[lin0.output], "h3") == N * K * 4 + (M + N) * K * 12 + M * N * 4
