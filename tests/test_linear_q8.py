"""Int8 weight-only decoder tenants (CPU): the row quantizer, the ``i8`` wire
dtype and the ``linear_q8`` op through validator, eager reference, Llama
builder, the CPU pod server and admission.  Quantization is a storage
format: everything is compared against the dequantized weights
(``dequantized_llama``), never against the fp32 model."""
from __future__ import annotations

import copy
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nos_amd.models.llama_program import dequantized_llama, llama_config, llama_decode_programs, llama_model
from nos_amd.ops import tenant as T
from nos_amd.podserver import program as PG
from nos_amd.podserver.client import PodClient, PodServerError
from nos_amd.podserver.program import Builder, ProgramError, dequantize_rows_q8, quantize_rows_q8
from nos_amd.podserver.server import PodServer

PROMPT_LEN, NEW, MAX_LEN = 16, 32, 64
PROMPT_SEED = 2   # chosen so the dequantized fp64 reference's top-2 gap clears 1e-4 at every step (asserted below)


@pytest.fixture(scope="module")
def model():
    return llama_model(llama_config(False), 0)


@pytest.fixture(scope="module")
def deq(model):
    return dequantized_llama(model)


@pytest.fixture(scope="module")
def tenant_q8(model):
    return llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="int8")


@pytest.fixture(scope="module")
def tenant_f32(model):
    return llama_decode_programs(model, PROMPT_LEN, MAX_LEN)


# ------------------------------------------------------------------ 1. the quantizer
def test_quantizer_round_trips_within_half_a_step_and_is_deterministic():
    rng = np.random.default_rng(0)
    w = (rng.standard_normal((37, 48)) * rng.uniform(0.01, 30, (37, 1))).astype(np.float32)
    w[5] = 0.0                                    # an all-zero row
    w[6, 3] = -w[6].__abs__().max() * 2           # the row maximum negative: maps to -127, never -128
    q, s = quantize_rows_q8(w)
    assert q.dtype == np.int8 and q.shape == (37, 48) and s.dtype == np.float32 and s.shape == (37,)
    assert q.min() >= -127 and q.max() <= 127 and q[6, 3] == -127
    assert s[5] == 1.0 and not q[5].any()
    back = dequantize_rows_q8(q, s)
    assert back.dtype == np.float32 and back.shape == w.shape
    # |w - q s| <= s / 2, plus the fp32 roundings of w / s and q * s (a few ulp of |w| <= 127 s)
    assert np.all(np.abs(back.astype(np.float64) - w) <= s[:, None].astype(np.float64) * (0.5 + 127 * 2.0 ** -22))
    q2, s2 = quantize_rows_q8(w.copy())
    assert np.array_equal(q, q2) and np.array_equal(s, s2)
    assert np.array_equal(np.abs(q).max(axis=1)[np.arange(37) != 5], np.full(36, 127))


# ------------------------------------------------------------------ 2. the validator
def _q8_program(k: int = 64, n: int = 24, x_dtype: str = "fp32", bias: bool = True):
    rng = np.random.default_rng(1)
    b = Builder("q8")
    x = b.input("x", [3, k], "fp32")
    if x_dtype != "fp32":
        x = b.op("cast", x, dtype=x_dtype)
    wq, sc = b.param_q8("w", rng.standard_normal((n, k)))
    ins = [x, wq, sc] + ([b.param("bias", rng.standard_normal(n))] if bias else [])
    y = b.op("linear_q8", *ins, act="gelu", out="y")
    return b.build([y])


def test_validator_accepts_a_well_formed_linear_q8():
    prog, w = _q8_program()
    p = PG.parse(prog, w, gpu=True)
    assert p.values["y"].shape == (3, 24) and p.values["y"].dtype == "fp32"
    assert p.params["w.q8"].dtype == "i8" and p.params["w.q8"].nbytes == 24 * 64
    assert p.param_bytes == 24 * 64 + 24 * 4 + 24 * 4
    t = p.tensors("cpu")
    assert t["w.q8"].dtype == torch.int8 and PG.torch_dtype("i8") == torch.int8
    assert "linear_q8" in PG.OPS and "linear_q8" in PG.NATIVE_KINDS and "linear_q8" in PG.NEVER_FOLD


def _mutated(mutate, **kw):
    prog, w = _q8_program(**kw)
    prog = copy.deepcopy(prog)
    mutate(prog)
    return prog, w


def _node(prog, op):
    return next(n for n in prog["nodes"] if n["op"] == op)


def _use_in_linear(p):
    _node(p, "linear_q8").update(op="linear", inputs=["x", "w.q8"])


def _use_in_embedding(p):
    p["inputs"][0].update(dtype="i32")
    _node(p, "linear_q8").update(op="embedding", inputs=["x", "w.q8"], attrs={})


def _wrong_scale(p):
    sc = next(q for q in p["params"] if q["name"] == "w.scale")
    sc.update(shape=[12, 2])


def _nbytes_mismatch(p):
    next(q for q in p["params"] if q["name"] == "w.q8").update(nbytes=24 * 64 * 4)


@pytest.mark.parametrize("mutate, match", [
    (_use_in_linear, "i8"),
    (_use_in_embedding, "i8"),
    (lambda p: p["outputs"].append("w.q8"), "i8"),
    (lambda p: p["inputs"][0].update(dtype="i8"), "input dtype"),
    (lambda p: p.update(state=[{"name": "s", "shape": [4], "dtype": "i8"}]), "state dtype"),
    (_wrong_scale, "wscale"),
    (_nbytes_mismatch, "nbytes"),
], ids=["i8-in-linear", "i8-in-embedding", "i8-output", "i8-input", "i8-state", "wscale-shape", "nbytes"])
def test_validator_refusals(mutate, match):
    prog, w = _mutated(mutate)
    with pytest.raises(ProgramError, match=match):
        PG.parse(prog, w)


def test_validator_names_the_node_that_misuses_an_i8_value():
    prog, w = _mutated(_use_in_linear)
    with pytest.raises(ProgramError, match=r"'y' \(linear\)"):
        PG.parse(prog, w)


def test_validator_refuses_a_bf16_x_and_k_48_on_the_gpu():
    prog, w = _q8_program(x_dtype="bf16")
    with pytest.raises(ProgramError, match="fp32"):
        PG.parse(prog, w)
    prog, w = _q8_program(k=48)
    PG.parse(prog, w)                           # fine off the GPU
    with pytest.raises(ProgramError, match="K % 32"):
        PG.parse(prog, w, gpu=True)


# ------------------------------------------------------------------ 3. the eager reference
@pytest.mark.parametrize("bias", [False, True])
def test_reference_is_f_linear_on_the_dequantized_weight_bit_for_bit(bias):
    prog, w = _q8_program(bias=bias)
    _node(prog, "linear_q8")["attrs"] = {}
    p = PG.parse(prog, w)
    t = p.tensors("cpu")
    x = torch.randn(3, 64, generator=torch.Generator().manual_seed(2))
    wf = t["w.q8"].float() * t["w.scale"][:, None]
    want = F.linear(x, wf, t["bias"] if bias else None)
    assert torch.equal(p.reference(x)[0], want)
    assert torch.equal(p.compile("cpu")(x)[0], want)
    assert torch.equal(T.linear_q8(x, t["w.q8"], t["w.scale"], t["bias"] if bias else None), want)
    assert np.array_equal(wf.numpy(), dequantize_rows_q8(t["w.q8"].numpy(), t["w.scale"].numpy()))
    ref64 = T.linear_q8_ref(x, t["w.q8"], t["w.scale"], t["bias"] if bias else None, dtype=torch.float64)
    assert ref64.dtype == torch.float64 and float((ref64 - want.double()).abs().max()) < 1e-5
    # the full int8 range is legal on the wire (the builder's quantizer never emits -128)
    q = t["w.q8"].clone()
    q[0, 0] = -128
    assert float(T.linear_q8(torch.eye(64)[:1], q, t["w.scale"])[0, 0]) == -128 * float(t["w.scale"][0])


def test_linear_q8_is_never_folded_into_an_fp32_weight():
    """All of its inputs constant: still a step (folding would materialise the fp32 weight)."""
    b = Builder("const")
    x = b.input("x", [1, 64], "fp32")
    c = b.param("c", np.ones((2, 64), np.float32))
    wq, sc = b.param_q8("w", np.random.default_rng(0).standard_normal((8, 64)))
    y = b.op("add", b.op("linear_q8", c, wq, sc), b.op("slice", x, dim=-1, start=0, end=8))
    prog, w = b.build([y])
    p = PG.parse(prog, w)
    assert not p.foldable()
    cp = p.compile("cpu")
    assert cp.stats["constant_folded"] == 0 and cp.stats["q8_linears"] == 1
    assert cp.consts["w.q8"].dtype == torch.int8 and not any(v.dtype == torch.float32 and v.shape == (8, 64)
                                                              for v in cp.consts.values())


# ------------------------------------------------------------------ 4. the Llama builder
def test_llama_int8_programs_share_one_smaller_payload(model, tenant_q8, tenant_f32):
    progs, w = tenant_q8
    ps = PG.parse_variants(progs, w)
    assert [p.inputs[0].shape for p in ps] == [(1, PROMPT_LEN), (1, 1)]
    q8 = [v for v in ps[0].params.values() if v.dtype == "i8"]
    cfg = model.config
    assert len(q8) == 4 * cfg.num_hidden_layers + 1          # qkv, o, gate_up, down per layer + the head
    assert ps[0].params["model.embed_tokens.weight"].dtype == "fp32"
    assert not any(n.op == "linear" for p in ps for n in p.nodes)
    # 3 bytes saved per quantized weight, less the one fp32 scale per row that the format adds: exactly
    # (the saving cannot exceed 3 bytes per weight; 4 bytes per row is 4 / K of a weight's byte)
    nq, rows = sum(v.numel for v in q8), sum(v.shape[0] for v in q8)
    assert len(tenant_f32[1]) - len(w) == 3 * nq - 4 * rows
    assert len(tenant_f32[1]) - len(w) > 2.9 * nq
    # the default is today's tenant, byte for byte
    assert llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="fp32")[1] == tenant_f32[1]
    assert json.dumps(llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="fp32")[0]) == json.dumps(tenant_f32[0])
    assert not any(v["dtype"] == "i8" for p in tenant_f32[0] for v in p["params"])
    with pytest.raises(ValueError, match="fp32"):
        llama_decode_programs(model, PROMPT_LEN, MAX_LEN, dtype="bf16", weights="int8")
    with pytest.raises(ValueError, match="weights"):
        llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="int4")


def test_a_tied_head_gets_its_own_quantized_copy():
    m = llama_model(llama_config(False, tie_word_embeddings=True, num_hidden_layers=1), 0)
    progs, w = llama_decode_programs(m, 4, 16, weights="int8")
    p = PG.parse_variants(progs, w)[0]
    assert p.params["model.embed_tokens.weight"].dtype == "fp32" and p.params["lm_head.weight.q8"].dtype == "i8"
    d = dequantized_llama(m)
    assert torch.equal(d.model.embed_tokens.weight, m.model.embed_tokens.weight)
    assert not torch.equal(d.lm_head.weight, m.lm_head.weight)
    ids = torch.randint(0, 512, (1, 4), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = d(ids).logits[:, -1:]
    got = p.reference(ids.int())[0]
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_compiled_decode_step_keeps_the_rms_prologue_and_epilogues(tenant_q8):
    ps = PG.parse_variants(*tenant_q8)
    c = ps[1].compile("cpu", params=ps[0].tensors("cpu"))
    layers = sum(1 for n in ps[1].nodes if n.op == "sdpa_cache")
    assert c.stats["q8_linears"] == 4 * layers + 1 and c.stats["q8_rms_prologue"] == 2 * layers + 1
    assert c.stats["rmsnorm_folded"] == 0 and c.stats["linears_merged"] == 0
    assert c.stats["residual_fused"] == 2 * layers
    kinds = [s.kind for s in c.steps]
    assert "rmsnorm" not in kinds and "add" not in kinds and "linear" not in kinds
    assert all(v.dtype != torch.float32 or v.dim() != 2 or k.startswith(("rope.", "model.embed"))
               for k, v in c.consts.items()), "no fp32 copy of a quantized weight"


# ------------------------------------------------------------------ 5. the CPU pod server
def _prompt() -> np.ndarray:
    return np.random.default_rng(PROMPT_SEED).integers(0, 512, (1, PROMPT_LEN)).astype(np.int32)


def reference_ids_and_gap(deq) -> tuple[np.ndarray, float]:
    """Greedy ids of the dequantized model in fp64, and the smallest top-2
    logit gap over the generated steps relative to the largest |logit|."""
    m64 = copy.deepcopy(deq).double()
    seq = torch.from_numpy(_prompt().astype(np.int64))
    gap = float("inf")
    with torch.no_grad():
        for _ in range(NEW):
            logits = m64(seq).logits[0, -1]
            top = logits.topk(2)
            gap = min(gap, float((top.values[0] - top.values[1]) / logits.abs().max()))
            seq = torch.cat([seq, top.indices[:1].view(1, 1)], 1)
    return seq[:, PROMPT_LEN:].numpy(), gap


def test_cpu_server_generates_the_dequantized_models_tokens(deq, tenant_q8, tmp_path):
    want, gap = reference_ids_and_gap(deq)
    assert gap >= 1e-4, f"top-2 gap {gap}: pick another PROMPT_SEED (the test must not ride on a near tie)"
    hf = deq.generate(torch.from_numpy(_prompt().astype(np.int64)), max_new_tokens=NEW, min_new_tokens=NEW,
                      do_sample=False, pad_token_id=0)[:, PROMPT_LEN:].numpy()
    assert np.array_equal(hf, want)
    progs, w = tenant_q8
    srv = PodServer(tmp_path / "s.sock", device="cpu", lanes=2, memory_gb=40).start()
    try:
        c = PodClient(srv.path, connect_timeout_s=5)
        c.register("llm-q8", progs[0], w, memory_limit_gb=1, variants=progs[1:])
        a, ta = c.generate(_prompt(), NEW, server_loop=True)
        b, tb = c.generate(_prompt(), NEW, server_loop=False)
        assert np.array_equal(a, want) and np.array_equal(b, want)
        assert ta["state"] == tb["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
        c.close()
    finally:
        srv.stop()


# ------------------------------------------------------------------ 6. admission
def _need(progs, kernel_config) -> int:
    """The server's static estimate of a tenant's variants (the weights and the state once)."""
    return (sum(p.bytes_estimate_for(kernel_config) for p in progs)
            - (len(progs) - 1) * (progs[0].param_bytes + progs[0].state_bytes))


def test_the_int8_tenant_fits_a_slice_the_fp32_tenant_does_not(tenant_q8, tenant_f32, tmp_path):
    pq, pf = PG.parse_variants(*tenant_q8), PG.parse_variants(*tenant_f32)
    assert pq[1].bytes_estimate_for(None) < pf[1].bytes_estimate_for(None)
    assert pq[1].param_bytes < pf[1].param_bytes
    # a decode step (1 row) needs no workspace for its int8 linears; a prefill dequantizes one weight at a time
    lin = next(n for n in pq[1].nodes if n.op == "linear_q8")
    ins = [pq[1].values[i] for i in lin.inputs]
    assert PG._workspace(lin, ins, pq[1].values[lin.output], "h3") == 0
    lin0 = next(n for n in pq[0].nodes if n.op == "linear_q8")
    ins0 = [pq[0].values[i] for i in lin0.inputs]
    assert PG._workspace(lin0, ins0, pq[0].values[lin0.output], "h3") > ins0[1].numel * 4
    srv = PodServer(tmp_path / "s.sock", device="cpu", lanes=2, memory_gb=40).start()
    try:
        nq, nf = _need(pq, srv.kernel_config), _need(pf, srv.kernel_config)
        assert nq < nf
        limit = (nq + nf) / 2 / 2 ** 30
        c = PodClient(srv.path, connect_timeout_s=5)
        with pytest.raises(PodServerError, match="static estimate") as e:
            c.register("llm-f32", tenant_f32[0][0], tenant_f32[1], memory_limit_gb=limit, variants=tenant_f32[0][1:])
        assert "AdmissionError" in str(e.value)
        c.close()
        c = PodClient(srv.path, connect_timeout_s=5)
        rep = c.register("llm-q8", tenant_q8[0][0], tenant_q8[1], memory_limit_gb=limit, variants=tenant_q8[0][1:])
        assert rep["ok"]
        c.close()
    finally:
        srv.stop()
