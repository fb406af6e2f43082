"""Quantized experts for mixture-of-experts tenants (CPU): the ``moe_q8`` / ``moe_mx4`` ops through
validator, eager reference, 3-D ``param_q8`` / ``param_mx4``, the ``experts=`` option of
``llama_decode_programs``, the static estimate, the registration's scale check and the CPU pod server,
against ``dequantized_llama(model, experts=...)`` in fp64.

Routing and the greedy choice are discontinuous: the reference ids come from ``test_moe.reference_run``,
which asserts the routing gap and the top-2 logit gap on the fp64 reference alone."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from nos_amd.models.llama_program import (dequantized_llama, llama_config, llama_decode_programs, llama_model,
                                          mixtral_config, mixtral_model)
from nos_amd.ops import tenant as T
from nos_amd.podserver import program as PG
from nos_amd.podserver.client import PodClient, PodServerError
from nos_amd.podserver.program import (Builder, ProgramError, dequantize_rows_mx4, dequantize_rows_q8,
                                       quantize_rows_mx4, quantize_rows_q8)
from nos_amd.podserver.program.reference import _eager
from nos_amd.podserver.server import PodServer
from test_moe import MAX_LEN, MODEL_SEED, NEW, PROMPT_LEN, make_qv_adapter, prompt, reference_run

FORMATS = ("int8", "mxfp4")
OP = {"int8": "moe_q8", "mxfp4": "moe_mx4"}


@pytest.fixture(scope="module")
def model():
    return mixtral_model(mixtral_config(), MODEL_SEED)


@pytest.fixture(scope="module")
def references(model):
    """Per format: the dequantized-experts model and its fp64 greedy ids of ``prompt(2)`` (both gaps asserted)."""
    out = {}
    for fmt in FORMATS:
        dm = dequantized_llama(model, experts=fmt)
        two = reference_run(dm, prompt(2))
        assert np.array_equal(reference_run(dm, prompt()), two[:1])
        out[fmt] = (dm, two)
    return out


# ------------------------------------------------------------------ 1. the validator
def _program(fmt="int8", E=4, H=64, I=32, k=2, rows=(2, 3), x_dtype="fp32", shapes=None, raw=None):
    """A one-node program over random experts; ``shapes``: other expert shapes before quantization; ``raw``:
    {input slot: (name, array, dtype)} params that replace a quantized operand as they are."""
    rng = np.random.default_rng(1)
    b = Builder("moe-quant")
    x = b.input("x", [*rows, H], "fp32")
    if x_dtype != "fp32":
        x = b.op("cast", x, dtype=x_dtype)
    s = shapes or {}
    wr = b.param("wr", rng.standard_normal(s.get("wr", (E, H))))
    quantized = b.param_q8 if fmt == "int8" else b.param_mx4
    ins = [x, wr, *quantized("w13", rng.standard_normal(s.get("w13", (E, 2 * I, H)))),
           *quantized("w2", rng.standard_normal(s.get("w2", (E, H, I))))]
    for slot, (name, a, dt) in (raw or {}).items():
        ins[slot] = b._param_u8(name, a) if dt == "u8" else b.param(name, a, dt)
    node = b.moe_q8 if fmt == "int8" else b.moe_mx4
    return b.build([node(*ins, k, out="y")])


@pytest.mark.parametrize("fmt", FORMATS)
def test_validator_accepts_a_well_formed_program(fmt):
    prog, w = _program(fmt)
    p = PG.parse(prog, w, gpu=True)
    assert p.values["y"].shape == (2, 3, 64) and p.values["y"].dtype == "fp32"
    assert OP[fmt] in PG.OPS and OP[fmt] in PG.NEVER_FOLD and p.foldable() == set()
    assert all(k in PG.NATIVE_KINDS for k in ("moe_glu_q8", "moe_down_q8", "moe_glu_mx4", "moe_down_mx4"))
    names = {q["name"]: (q["shape"], q["dtype"]) for q in prog["params"]}
    if fmt == "int8":
        assert names["w13.q8"] == ([4, 64, 64], "i8") and names["w13.scale"] == ([4, 64], "fp32")
        assert names["w2.q8"] == ([4, 64, 32], "i8") and names["w2.scale"] == ([4, 64], "fp32")
    else:
        assert names["w13.mx4"] == ([4, 64, 32], "u8") and names["w13.e8m0"] == ([4, 64, 2], "u8")
        assert names["w2.mx4"] == ([4, 64, 16], "u8") and names["w2.e8m0"] == ([4, 64, 1], "u8")


@pytest.mark.parametrize("fmt, kw, match", [
    ("int8", dict(k=0), "top_k"), ("mxfp4", dict(k=0), "top_k"),
    ("int8", dict(k=5), "top_k"), ("mxfp4", dict(k=5), "top_k"),                 # k > E = 4
    ("int8", dict(E=16, k=9), "top_k"), ("mxfp4", dict(E=16, k=9), "top_k"),     # k > 8
    ("int8", dict(E=65), "E <= 64"), ("mxfp4", dict(E=65), "E <= 64"),
    ("int8", dict(H=72), "H % 16 == 0"), ("int8", dict(I=24), "I % 16 == 0"),
    ("mxfp4", dict(H=96 + 16, shapes={"w13": (4, 64, 96), "w2": (4, 96 + 16, 32)}), "shapes must match"),
    ("mxfp4", dict(H=32, I=48, shapes={"w13": (4, 96, 32), "w2": (4, 32, 64)}), "shapes must match"),
    ("int8", dict(shapes={"wr": (3, 64)}), "shapes must match"),
    ("int8", dict(shapes={"w13": (4, 64, 48)}), "shapes must match"),
    ("int8", dict(shapes={"w2": (4, 64, 16)}), "shapes must match"),
    ("int8", dict(shapes={"w2": (4, 32, 64)}), "shapes must match"),
    ("mxfp4", dict(shapes={"w13": (4, 64, 32)}), "shapes must match"),
    ("mxfp4", dict(shapes={"w2": (4, 64, 64)}), "shapes must match"),
    ("int8", dict(x_dtype="bf16"), "x must be fp32"), ("mxfp4", dict(x_dtype="bf16"), "x must be fp32"),
    # the scales' shapes follow the codes'
    ("int8", dict(raw={3: ("s13", np.ones((4, 32), np.float32), "fp32")}), "scales' shapes must match"),
    ("mxfp4", dict(raw={5: ("e2", np.full((4, 64, 2), 127, np.uint8), "u8")}), "scales' shapes must match"),
    # wrong dtypes: fp32 codes, fp32 MXFP4 scales, u8 int8 scales
    ("int8", dict(raw={2: ("w13f", np.ones((4, 64, 64), np.float32), "fp32")}), "must be i8 params"),
    ("mxfp4", dict(raw={4: ("w2f", np.ones((4, 64, 16), np.float32), "fp32")}), "must be u8 params"),
    ("mxfp4", dict(raw={3: ("e13f", np.ones((4, 64, 2), np.float32), "fp32")}), "scales must be u8 params"),
])
def test_validator_refuses(fmt, kw, match):
    prog, w = _program(fmt, **kw)
    with pytest.raises(ProgramError, match=match):
        PG.parse(prog, w, gpu=False)


def test_validator_refuses_the_mx4_block_rule_and_the_other_formats_codes():
    # H = 48 and I = 48: multiples of 16 (int8 takes them), no multiples of 32
    PG.parse(*_program("int8", H=48, I=48))
    rng = np.random.default_rng(2)
    for H, I, match in ((48, 32, "H % 32 == 0"), (32, 48, "I % 32 == 0")):
        b = Builder("moe-mx4-off")
        x = b.input("x", [2, H], "fp32")
        ins = [x, b.param("wr", rng.standard_normal((4, H))),
               b._param_u8("c13", np.zeros((4, 2 * I, H // 2), np.uint8)), b._param_u8("e13", np.full((4, 2 * I, max(H // 32, 1)), 127, np.uint8)),
               b._param_u8("c2", np.zeros((4, H, I // 2), np.uint8)), b._param_u8("e2", np.full((4, H, max(I // 32, 1)), 127, np.uint8))]
        with pytest.raises(ProgramError, match=match):
            PG.parse(*b.build([b.moe_mx4(*ins, 2, out="y")]))
    # an i8 param is the weight of linear_q8 or the codes of moe_q8, nothing else; a u8 param likewise
    prog, w = _program("int8")
    node = next(n for n in prog["nodes"] if n["op"] == "moe_q8")
    node["inputs"][1], node["inputs"][2] = node["inputs"][2], node["inputs"][1]
    with pytest.raises(ProgramError, match="i8 param"):
        PG.parse(prog, w)
    prog, w = _program("mxfp4")
    node = next(n for n in prog["nodes"] if n["op"] == "moe_mx4")
    node["inputs"][1], node["inputs"][2] = node["inputs"][2], node["inputs"][1]
    with pytest.raises(ProgramError, match="u8 param"):
        PG.parse(prog, w)


@pytest.mark.parametrize("fmt", FORMATS)
def test_validator_refuses_weights_that_are_not_params_and_unknown_attributes(fmt):
    prog, w = _program(fmt)
    node = next(n for n in prog["nodes"] if n["op"] == OP[fmt])
    prog["nodes"].insert(0, {"op": "mul", "inputs": ["wr", "wr"], "output": "wr2", "attrs": {}})
    node["inputs"][1] = "wr2"
    with pytest.raises(ProgramError, match="must be an fp32 param"):
        PG.parse(prog, w)
    if fmt == "int8":   # a computed scale
        prog, w = _program(fmt)
        node = next(n for n in prog["nodes"] if n["op"] == OP[fmt])
        prog["nodes"].insert(0, {"op": "mul", "inputs": ["w2.scale", "w2.scale"], "output": "s2", "attrs": {}})
        node["inputs"][5] = "s2"
        with pytest.raises(ProgramError, match="scales must be fp32 params"):
            PG.parse(prog, w)
    prog, w = _program(fmt)
    next(n for n in prog["nodes"] if n["op"] == OP[fmt])["attrs"]["renorm"] = True
    with pytest.raises(ProgramError, match="unknown attributes"):
        PG.parse(prog, w)
    prog, w = _program(fmt)
    next(n for n in prog["nodes"] if n["op"] == OP[fmt])["inputs"].pop()
    with pytest.raises(ProgramError):
        PG.parse(prog, w)


# ------------------------------------------------------------------ 2. the eager reference, the 3-D params
@pytest.mark.parametrize("fmt", FORMATS)
def test_eager_reference_is_moe_ref_on_the_dequantized_experts_bit_for_bit(fmt):
    prog, w = _program(fmt, rows=(7, 1))
    p = PG.parse(prog, w)
    t = p.tensors("cpu")
    if fmt == "int8":
        deq = lambda n: torch.from_numpy(np.stack([dequantize_rows_q8(q, s) for q, s in  # noqa: E731
                                                   zip(t[n + ".q8"].numpy(), t[n + ".scale"].numpy())]))
        args = [t["wr"], t["w13.q8"], t["w13.scale"], t["w2.q8"], t["w2.scale"]]
    else:
        deq = lambda n: torch.from_numpy(np.stack([dequantize_rows_mx4(c, e) for c, e in  # noqa: E731
                                                   zip(t[n + ".mx4"].numpy(), t[n + ".e8m0"].numpy())]))
        args = [t["wr"], t["w13.mx4"], t["w13.e8m0"], t["w2.mx4"], t["w2.e8m0"]]
    W13, W2 = deq("w13"), deq("w2")
    assert W13.dtype == torch.float32
    x = torch.randn(7, 1, 64, generator=torch.Generator().manual_seed(3))
    want = T.moe_ref(x, t["wr"], W13, W2, 2)
    assert torch.equal(_eager(OP[fmt], [x, *args], {"top_k": 2}), want)
    assert torch.equal(p.reference(x)[0], want)
    assert torch.equal((T.moe_q8 if fmt == "int8" else T.moe_mx4)(x, *args, 2), want)   # CPU tensors: the reference
    # in fp64: the experts are formed in fp32 (the format's definition), the arithmetic runs in x's dtype
    want64 = T.moe_ref(x.double(), t["wr"].double(), W13.double(), W2.double(), 2)
    got64 = _eager(OP[fmt], [x.double(), t["wr"].double(), *args[1:]], {"top_k": 2})
    assert got64.dtype == torch.float64 and torch.equal(got64, want64)
    # the kernels' wrappers on CPU tensors are the per-launch references
    idx, wts = T.moe_route_ref(x.view(7, 64), t["wr"], 2)
    glu = T.moe_glu_q8 if fmt == "int8" else T.moe_glu_mx4
    down = T.moe_down_q8 if fmt == "int8" else T.moe_down_mx4
    act = glu(x.view(7, 64), idx, args[1], args[2])
    assert torch.equal(act, T.moe_glu_ref(x.view(7, 64), idx, W13))
    assert torch.equal(down(act, idx, wts, args[3], args[4]).view(7, 1, 64), want)


def test_3d_params_are_the_2d_functions_on_the_flattened_rows():
    rng = np.random.default_rng(4)
    w3 = rng.standard_normal((3, 10, 64)).astype(np.float32)
    w3[1, 2] = 0.0                                   # an all-zero row: scale 1, block scale 127
    w2d = w3.reshape(30, 64)
    b = Builder("p")
    names = [*b.param_q8("a", w3), *b.param_mx4("a", w3), *b.param_q8("f", w2d), *b.param_mx4("f", w2d)]
    assert names == ["a.q8", "a.scale", "a.mx4", "a.e8m0", "f.q8", "f.scale", "f.mx4", "f.e8m0"]
    prog, raw = b.build(["a.q8"])
    ps = {p["name"]: p for p in prog["params"]}

    def data(n):
        return raw[ps[n]["offset"]:ps[n]["offset"] + ps[n]["nbytes"]]

    q, s = quantize_rows_q8(w2d)
    c, e = quantize_rows_mx4(w2d)
    assert (ps["a.q8"]["shape"], ps["a.q8"]["dtype"]) == ([3, 10, 64], "i8") and data("a.q8") == q.tobytes()
    assert (ps["a.scale"]["shape"], ps["a.scale"]["dtype"]) == ([3, 10], "fp32") and data("a.scale") == s.tobytes()
    assert (ps["a.mx4"]["shape"], ps["a.mx4"]["dtype"]) == ([3, 10, 32], "u8") and data("a.mx4") == c.tobytes()
    assert (ps["a.e8m0"]["shape"], ps["a.e8m0"]["dtype"]) == ([3, 10, 2], "u8") and data("a.e8m0") == e.tobytes()
    # 2-D calls: the shapes and bytes they have always produced
    assert ps["f.q8"]["shape"] == [30, 64] and data("f.q8") == q.tobytes()
    assert ps["f.scale"]["shape"] == [30] and data("f.scale") == s.tobytes()
    assert ps["f.mx4"]["shape"] == [30, 32] and data("f.mx4") == c.tobytes()
    assert ps["f.e8m0"]["shape"] == [30, 2] and data("f.e8m0") == e.tobytes()
    assert all(ps[n]["offset"] % 4 == 0 for n in ps)
    with pytest.raises(ValueError):
        b.param_q8("bad", np.zeros((2, 2, 2, 16), np.float32))
    with pytest.raises(ValueError, match="K % 32"):
        b.param_mx4("bad", np.zeros((2, 2, 48), np.float32))


# ------------------------------------------------------------------ 3. the builder
def test_experts_values_names_and_refusals(model):
    def build(m=model, **kw):
        return llama_decode_programs(m, PROMPT_LEN, MAX_LEN, **kw)

    plain = build()
    assert build(experts="fp32") == plain                      # programs and payload, byte for byte
    for fmt, tag in (("int8", "eq8"), ("mxfp4", "emx4")):
        progs, _ = build(experts=fmt)
        assert [p["name"] for p in progs] == [f"mixtral-h256-l2-fp32-{tag}-prefill8", f"mixtral-h256-l2-fp32-{tag}-step1"]
        ops = [n["op"] for n in progs[1]["nodes"]]
        assert ops.count(OP[fmt]) == 2 and "moe" not in ops and "linear_q8" not in ops and "linear_mx4" not in ops
        by = {p["name"]: p["dtype"] for p in progs[1]["params"]}
        assert by["model.layers.0.mlp.gate.weight"] == "fp32" and by["model.embed_tokens.weight"] == "fp32"
        assert by["model.layers.0.self_attn.q_proj.weight"] == "fp32"
        PG.parse_variants(progs, _, gpu=True)
    assert build(experts="int8", kv="int8", speculate=4)[0][-1]["name"] == "mixtral-h256-l2-fp32-eq8-kvq8-spec-verify4"
    # beside everything else a Mixtral tenant takes
    progs, w = build(experts="mxfp4", batch=2, extend=(4,), sampling=True, stopping=True, kv="int8",
                     adapters=[make_qv_adapter(model)])
    assert progs[1]["name"] == "mixtral-h256-l2-fp32-emx4-kvq8-stop-lora-step1"
    assert len(PG.parse_variants(progs, w, gpu=True)) == 3
    for bad in ("fp16", "q8", None, 8):
        with pytest.raises(ValueError, match="experts must be 'fp32', 'int8' or 'mxfp4'"):
            build(experts=bad)
    dense = llama_model(llama_config(), 0)
    for fmt in FORMATS:
        with pytest.raises(ValueError, match="is a Mixtral tenant's option"):
            build(dense, experts=fmt)
        with pytest.raises(ValueError, match="dtype='bf16' is not taken"):
            build(experts=fmt, dtype="bf16")
    build(dense, experts="fp32")
    # weights= on a Mixtral stays refused, with or without experts=
    with pytest.raises(ValueError, match="weights='int8' is not taken"):
        build(weights="int8")
    with pytest.raises(ValueError, match="weights='mxfp4' is not taken"):
        build(weights="mxfp4", experts="mxfp4")
    # the divisibility rules, by name
    h264 = mixtral_model(mixtral_config(num_hidden_layers=1, hidden_size=264, num_attention_heads=2,
                                        num_key_value_heads=1, head_dim=128, vocab_size=32), MODEL_SEED)
    with pytest.raises(ValueError, match=r"experts='int8': hidden_size = 264 is not a multiple of 16"):
        build(h264, experts="int8")
    i104 = mixtral_model(mixtral_config(num_hidden_layers=1, intermediate_size=104, vocab_size=32), MODEL_SEED)
    with pytest.raises(ValueError, match=r"experts='int8': intermediate_size = 104 is not a multiple of 16"):
        build(i104, experts="int8")
    i112 = mixtral_model(mixtral_config(num_hidden_layers=1, intermediate_size=112, vocab_size=32), MODEL_SEED)
    build(i112, experts="int8")
    with pytest.raises(ValueError, match=r"experts='mxfp4': intermediate_size = 112 is not a multiple of 32"):
        build(i112, experts="mxfp4")
    h272 = mixtral_model(mixtral_config(num_hidden_layers=1, hidden_size=272, num_attention_heads=2,
                                        num_key_value_heads=1, head_dim=128, vocab_size=32), MODEL_SEED)
    with pytest.raises(ValueError, match=r"experts='mxfp4': hidden_size = 272 is not a multiple of 32"):
        build(h272, experts="mxfp4")
    with pytest.raises(ValueError, match="experts must be 'int8' or 'mxfp4'"):
        dequantized_llama(model, experts="fp32")


def test_dequantized_llama_roundtrips_the_expert_tensors_only(model):
    sd = model.state_dict()
    for fmt in FORMATS:
        dq = dequantized_llama(model, experts=fmt).state_dict()
        rt = (lambda w: dequantize_rows_q8(*quantize_rows_q8(w))) if fmt == "int8" else \
            (lambda w: dequantize_rows_mx4(*quantize_rows_mx4(w)))
        changed = 0
        for k, v in sd.items():
            if k.endswith(("mlp.experts.gate_up_proj", "mlp.experts.down_proj")):
                w = v.numpy()
                assert np.array_equal(dq[k].numpy(), rt(w.reshape(-1, w.shape[-1])).reshape(w.shape)), k
                assert not torch.equal(dq[k], v)
                changed += 1
            else:
                assert torch.equal(dq[k], v), k
        assert changed == 2 * model.config.num_hidden_layers
    # without the keyword: the dense model's behaviour, unchanged (a Mixtral's attention projections)
    dq = dequantized_llama(model).state_dict()
    assert torch.equal(dq["model.layers.0.mlp.experts.down_proj"], sd["model.layers.0.mlp.experts.down_proj"])
    assert not torch.equal(dq["model.layers.0.self_attn.q_proj.weight"], sd["model.layers.0.self_attn.q_proj.weight"])


def test_payload_sizes_are_exact(model):
    cfg = model.config
    L, E, H, I = cfg.num_hidden_layers, cfg.num_local_experts, cfg.hidden_size, cfg.intermediate_size
    fp32 = len(llama_decode_programs(model, PROMPT_LEN, MAX_LEN)[1])
    experts_fp32 = L * E * 3 * H * I * 4
    want = {"int8": fp32 - experts_fp32 + L * E * (3 * H * I + (2 * I + H) * 4),
            "mxfp4": fp32 - experts_fp32 + L * E * (3 * H * I // 2 + 3 * H * I // 32)}
    for fmt in FORMATS:
        progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, experts=fmt)
        assert len(w) == want[fmt], fmt
        assert PG.parse_variants(progs, w)[0].param_bytes == len(w)   # no padding between the params here


def test_static_estimate_counts_the_stored_bytes_and_one_transient_expert():
    H, I = 256, 96
    stored = {"fp32": 3 * H * I * 4, "int8": 3 * H * I + (2 * I + H) * 4, "mxfp4": 3 * H * I // 2 + 3 * H * I // 32}
    est = {}
    for fmt in ("fp32", *FORMATS):
        for E in (4, 8):
            m = mixtral_model(mixtral_config(num_local_experts=E), MODEL_SEED)
            progs, w = llama_decode_programs(m, PROMPT_LEN, MAX_LEN, extend=(16,), experts=fmt)
            ps = PG.parse_variants(progs, w)
            est[fmt, E] = [(p.bytes_estimate, p.param_bytes) for p in ps]
            assert ps[0].param_bytes == len(w)
    one = (2 * I * H + H * I) * 4                     # one expert's two tensors in fp32
    for fmt in FORMATS:
        per_expert = 2 * (H * 4 + stored[fmt])        # two layers' router row and stored expert tensors
        for v in range(3):                            # prefill 8, step 1, extend 16
            (e4, p4), (e8, p8) = est[fmt, 4][v], est[fmt, 8][v]
            assert p8 - p4 == 4 * per_expert
            if v < 2:   # the kernels' transients hold no E
                assert e8 - e4 == 4 * per_expert
            else:       # the dense path: only the gates and the probabilities [rows, E] grow with E
                assert 4 * per_expert <= e8 - e4 <= 4 * per_expert + 2 * 16 * 3 * 4 * 4
            # against the fp32-expert tenant: the params shrink to their stored sizes; decode rows hold the same
            # scratch, 16 rows also the one-expert transient (twice: the graph's buffers and the solo run's)
            f, pf = est["fp32", 4][v]
            shrink = 2 * 4 * (stored["fp32"] - stored[fmt])
            assert pf - p4 == shrink
            if v < 2:
                assert f - e4 == shrink
            else:
                assert shrink - 2 * one <= f - e4 <= shrink and f - e4 < shrink


@pytest.mark.parametrize("byte", [1, 255])
def test_a_scale_byte_outside_2_to_252_in_an_expert_tensor_is_refused_at_registration(byte, tmp_path):
    prog, w = _program("mxfp4")
    for name in ("w13.e8m0", "w2.e8m0"):
        off = next(p for p in prog["params"] if p["name"] == name)["offset"]
        bad = bytearray(w)
        bad[off + 7] = byte
        p = PG.parse(prog, bytes(bad))
        with pytest.raises(ValueError, match=rf"param '{name}': MXFP4 block scale byte {byte} is outside \[2, 252\]"):
            p.tensors("cpu")
        for ok in (2, 252):
            bad[off + 7] = ok
            PG.parse(prog, bytes(bad)).tensors("cpu")
    bad[off + 7] = byte
    srv = PodServer(tmp_path / "s.sock", device="cpu", lanes=2, memory_gb=40).start()
    try:
        c = PodClient(srv.path, connect_timeout_s=5)
        with pytest.raises(PodServerError, match=f"w2.e8m0.*scale byte {byte}"):
            c.register("bad", prog, bytes(bad), memory_limit_gb=1)
        c.close()
    finally:
        srv.stop()


@pytest.mark.parametrize("fmt", FORMATS)
def test_training_tenants_refuse_the_quantized_ops(fmt):
    from nos_amd.podserver.training import parse_train_spec

    prog, w = _program(fmt)
    with pytest.raises(ProgramError, match=f"{OP[fmt]} node cannot be a training tenant"):
        parse_train_spec({"loss": "mse"}, PG.parse(prog, w))


# ------------------------------------------------------------------ 4. the CPU pod server
def _serve(tmp_path, name, progs, w):
    srv = PodServer(tmp_path / f"{name}.sock", device="cpu", lanes=2, memory_gb=40).start()
    c = PodClient(srv.path, connect_timeout_s=5)
    c.register(name, progs[0], w, memory_limit_gb=1, variants=progs[1:])
    return srv, c


@pytest.mark.parametrize("fmt", FORMATS)
def test_cpu_server_generates_the_dequantized_models_tokens(fmt, model, references, tmp_path):
    _, want = references[fmt]
    differs = int((want != reference_run(model, prompt(2))).sum())   # of the 32 tokens of prompt(2)
    if fmt == "mxfp4":   # the ids tell quantized experts from experts silently left fp32 (the batch-two test runs both rows)
        assert differs > 0
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, experts=fmt)
    srv, c = _serve(tmp_path, "moe-" + fmt, progs, w)
    try:
        for loop in (True, False):
            ids, t = c.generate(prompt(), NEW, server_loop=loop)
            assert np.array_equal(ids, want[:1]), (fmt, loop)
            assert t["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
            c.reset()
        if fmt == "int8":   # its ids cannot tell: the logits must differ from the fp32-expert tenant's
            assert differs == 0
            logits = c.infer(prompt(), outputs=[0])[0][0]
            plain, wp = llama_decode_programs(model, PROMPT_LEN, MAX_LEN)
            c2 = PodClient(srv.path, connect_timeout_s=5)
            c2.register("moe-fp32", plain[0], wp, memory_limit_gb=1, variants=plain[1:])
            base = c2.infer(prompt(), outputs=[0])[0][0]
            c2.close()
            assert logits.shape == base.shape and float(np.abs(logits - base).max()) > 1e-5 * float(np.abs(base).max())
        c.close()
    finally:
        srv.stop()


@pytest.mark.parametrize("fmt", FORMATS)
def test_cpu_server_batch_two_and_an_extend(fmt, model, references, tmp_path):
    _, want = references[fmt]
    progs, w = llama_decode_programs(model, PROMPT_LEN - 3, MAX_LEN, batch=2, extend=(3,), experts=fmt)
    srv, c = _serve(tmp_path, "moe-b2-" + fmt, progs, w)
    try:
        two = prompt(2)
        c.infer(two[:, :PROMPT_LEN - 3])
        outs, _ = c.infer(two[:, PROMPT_LEN - 3:], outputs=[1])   # the extend variant finishes the prompt
        toks = [outs[0].reshape(2, 1).astype(np.int32)]
        for _ in range(NEW - 1):
            outs, rep = c.infer(toks[-1], outputs=[1])
            toks.append(outs[0].reshape(2, 1).astype(np.int32))
        assert np.array_equal(np.concatenate(toks, 1), want)
        assert rep["state"] == {"pos": [PROMPT_LEN + NEW - 1] * 2}
        c.close()
    finally:
        srv.stop()
