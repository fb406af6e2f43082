"""Mixture-of-experts decoder tenants (CPU): the ``moe`` op through validator,
eager reference, static estimate, the Mixtral dispatch of
``llama_decode_programs`` and the CPU pod server, against transformers'
``MixtralSparseMoeBlock`` / ``MixtralForCausalLM``.

Routing and the greedy choice are discontinuous, so no test may sit on a tie:
``reference_run`` asserts, in fp64 alone, that the k-th and (k+1)-th router
probabilities differ by at least ``MIN_ROUTE_GAP`` at every row, layer and step
and that the top-2 logits differ by at least ``MIN_GAP`` of max |logit| at every
generated token.  A seed that misses either is replaced, never the bound."""
from __future__ import annotations

import copy
import hashlib
import json

import numpy as np
import pytest
import torch

from nos_amd.models.llama_program import (adapted_llama, llama_config, llama_decode_programs, llama_model,
                                          llama_program, mixtral_config, mixtral_model, rope_tables)
from nos_amd.ops import tenant as T
from nos_amd.podserver import program as PG
from nos_amd.podserver.client import PodClient
from nos_amd.podserver.program import Builder, ProgramError
from nos_amd.podserver.program.reference import _eager
from nos_amd.podserver.server import PodServer

PROMPT_LEN, NEW, MAX_LEN = 8, 16, 48
MODEL_SEED = 0
PROMPT_SEED = 8      # chosen so that reference_run's two gaps hold for every prompt the tests use
MIN_ROUTE_GAP = 1e-3
MIN_GAP = 1e-4       # tests/test_speculative.py MIN_GAP
PAD = 3


@pytest.fixture(scope="module")
def model():
    return mixtral_model(mixtral_config(), MODEL_SEED)


def prompt(rows: int = 1, seed: int = PROMPT_SEED, n: int = PROMPT_LEN) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 512, (rows, n)).astype(np.int32)


def reference_run(m, ids: np.ndarray, new: int = NEW):
    """Greedy ids [rows, new] of ``m`` in fp64 for the prompts ``ids``, with both conditions on the
    inputs asserted on this reference alone: the routing gap at every row, layer and step, the top-2
    logit gap at every generated token."""
    m64 = copy.deepcopy(m).double()
    k = m64.config.num_experts_per_tok
    route_gap = [float("inf")]

    def hook(_mod, _inp, out):   # out[0]: the router's logits [rows, E]
        p = torch.softmax(out[0].double(), -1).sort(-1, descending=True).values
        if p.shape[-1] > k:
            route_gap[0] = min(route_gap[0], float((p[:, k - 1] - p[:, k]).min()))

    hooks = [layer.mlp.gate.register_forward_hook(hook) for layer in m64.model.layers]
    seq = torch.from_numpy(ids.astype(np.int64))
    gap = float("inf")
    with torch.no_grad():
        for _ in range(new):
            logits = m64(seq).logits[:, -1]
            top = logits.topk(2, dim=-1)
            gap = min(gap, float(((top.values[:, 0] - top.values[:, 1]) / logits.abs().amax(-1)).min()))
            seq = torch.cat([seq, top.indices[:, :1]], 1)
    for h in hooks:
        h.remove()
    assert route_gap[0] >= MIN_ROUTE_GAP, f"routing gap {route_gap[0]}: pick another seed (no test may ride on a tie)"
    assert gap >= MIN_GAP, f"top-2 logit gap {gap}: pick another seed (no test may ride on a near tie)"
    return seq[:, ids.shape[1]:].numpy().astype(np.int32)


@pytest.fixture(scope="module")
def reference(model):
    """The fp64 greedy ids of ``prompt(2)`` (rows 0 and 1; row 0 is ``prompt()``), conditions asserted."""
    two = reference_run(model, prompt(2))
    one = reference_run(model, prompt())
    assert np.array_equal(one, two[:1])
    return two


# ------------------------------------------------------------------ 1. the validator
def _moe_program(E=4, H=32, I=24, k=2, rows=(2, 3), shapes=None, x_dtype="fp32"):
    rng = np.random.default_rng(1)
    b = Builder("moe")
    x = b.input("x", [*rows, H], "fp32")
    if x_dtype != "fp32":
        x = b.op("cast", x, dtype=x_dtype)
    s = shapes or {}
    wr = b.param("wr", rng.standard_normal(s.get("wr", (E, H))))
    w13 = b.param("w13", rng.standard_normal(s.get("w13", (E, 2 * I, H))))
    w2 = b.param("w2", rng.standard_normal(s.get("w2", (E, H, I))))
    return b.build([b.moe(x, wr, w13, w2, k, out="y")])


def test_validator_accepts_a_well_formed_moe_program():
    prog, w = _moe_program()
    p = PG.parse(prog, w, gpu=True)
    assert p.values["y"].shape == (2, 3, 32) and p.values["y"].dtype == "fp32"
    assert "moe" in PG.OPS and "moe" in PG.NEVER_FOLD
    assert all(k in PG.NATIVE_KINDS for k in ("moe_route", "moe_glu", "moe_down"))
    assert p.foldable() == set()


@pytest.mark.parametrize("kw, match", [
    (dict(k=0), "top_k"),
    (dict(k=5), "top_k"),                       # k > E = 4
    (dict(E=16, k=9), "top_k"),                 # k > 8
    (dict(E=65), "E <= 64"),
    (dict(H=30), "H % 4 == 0"),
    (dict(I=22), "I % 4 == 0"),
    (dict(shapes={"wr": (3, 32)}), "shapes must match"),
    (dict(shapes={"w13": (4, 48, 28)}), "shapes must match"),
    (dict(shapes={"w2": (4, 32, 20)}), "shapes must match"),
    (dict(shapes={"w2": (4, 24, 32)}), "shapes must match"),
    (dict(shapes={"w13": (4, 47, 32)}), "shapes must match"),
    (dict(x_dtype="bf16"), "x must be fp32"),
])
def test_validator_refuses(kw, match):
    prog, w = _moe_program(**kw)
    with pytest.raises(ProgramError, match=match):
        PG.parse(prog, w, gpu=False)


def test_validator_refuses_weights_that_are_not_params():
    prog, w = _moe_program()
    node = next(n for n in prog["nodes"] if n["op"] == "moe")
    prog["nodes"].insert(0, {"op": "mul", "inputs": ["wr", "wr"], "output": "wr2", "attrs": {}})
    node["inputs"][1] = "wr2"
    with pytest.raises(ProgramError, match="fp32 params"):
        PG.parse(prog, w)
    prog, w = _moe_program()
    next(n for n in prog["nodes"] if n["op"] == "moe")["attrs"]["renorm"] = True
    with pytest.raises(ProgramError, match="unknown attributes"):
        PG.parse(prog, w)


# ------------------------------------------------------------------ 2. the contract
def _literal_moe(x, Wr, W13, W2, k):
    """The issue's four steps, row by row, in x's dtype."""
    I = W13.shape[1] // 2
    out = torch.zeros_like(x)
    picks = []
    for m in range(x.shape[0]):
        p = torch.softmax(Wr @ x[m], -1)
        order = sorted(range(len(p)), key=lambda e: (-float(p[e]), e))[:k]   # a tie: the lower index
        tot = sum(p[e] for e in order)
        y = torch.zeros_like(x[m])
        for e in order:
            g, u = W13[e][:I] @ x[m], W13[e][I:] @ x[m]
            y = y + (p[e] / tot) * (W2[e] @ (torch.nn.functional.silu(g) * u))
        out[m] = y
        picks.append(order)
    return out, picks


@pytest.mark.parametrize("E, k, H, I", [(2, 1, 8, 4), (5, 2, 24, 12), (8, 8, 16, 20)])
def test_moe_ref_is_the_literal_loop(E, k, H, I):
    g = torch.Generator().manual_seed(E + k)
    x = torch.randn(7, H, generator=g, dtype=torch.float64)
    Wr, W13, W2 = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((E, H), (E, 2 * I, H), (E, H, I)))
    want, picks = _literal_moe(x, Wr, W13, W2, k)
    got = T.moe_ref(x.view(7, 1, H), Wr, W13, W2, k)
    assert got.dtype == torch.float64 and got.shape == (7, 1, H)
    assert float((got.view(7, H) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    idx, w = T.moe_route_ref(x, Wr, k, dtype=torch.float64)
    assert idx.dtype == torch.int32 and idx.tolist() == picks
    assert torch.allclose(w.sum(-1), torch.ones(7, dtype=torch.float64), atol=1e-14) and bool((w[:, :-1] >= w[:, 1:]).all())
    # fp32 inputs computed in fp64 on request (what the GPU tests compare against)
    up = T.moe_ref(x.float(), Wr.float(), W13.float(), W2.float(), k, dtype=torch.float64)
    assert up.dtype == torch.float64


def test_ties_go_to_the_lower_index():
    x = torch.zeros(2, 8)
    x[:, 0] = 1.0
    Wr = torch.zeros(4, 8)
    idx, w = T.moe_route_ref(x, Wr, 2)            # every p equal
    assert idx.tolist() == [[0, 1], [0, 1]] and w.tolist() == [[0.5, 0.5], [0.5, 0.5]]
    Wr[:, 0] = torch.tensor([0.0, 1.0, 0.0, 1.0])   # experts 1 and 3 tie for the top, 0 and 2 below
    idx, w = T.moe_route_ref(x, Wr, 3)
    assert idx.tolist() == [[1, 3, 0], [1, 3, 0]]
    idx, _ = T.moe_route(x, Wr, 1)                # the wrapper's CPU path is the reference
    assert idx.tolist() == [[1], [1]]
    # an index outside [0, E) contributes zero (and the reference reads no weight with it)
    W13, W2 = torch.randn(4, 8, 8), torch.randn(4, 8, 4)
    bad = torch.tensor([[1, 7], [-1, 2]], dtype=torch.int32)
    ws = torch.full((2, 2), 0.5)
    act = T.moe_glu(x, bad, W13)
    assert bool((act[0, 1] == 0).all()) and bool((act[1, 0] == 0).all()) and bool((act[0, 0] != 0).any())
    y = T.moe_down(torch.ones(2, 2, 4), bad, ws, W2)
    assert torch.allclose(y[0], 0.5 * W2[1].sum(-1)) and torch.allclose(y[1], 0.5 * W2[2].sum(-1))


def test_eager_reference_is_mixtral_sparse_moe_block_in_fp64(model):
    block = copy.deepcopy(model.model.layers[0].mlp).double()
    cfg = model.config
    x = torch.randn(2, 5, cfg.hidden_size, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    p = torch.softmax(x.view(-1, cfg.hidden_size) @ block.gate.weight.detach().T, -1).sort(-1, descending=True).values
    k = cfg.num_experts_per_tok
    assert float((p[:, k - 1] - p[:, k]).min()) >= MIN_ROUTE_GAP
    with torch.no_grad():
        want = block(x)
        got = _eager("moe", [x, block.gate.weight, block.experts.gate_up_proj, block.experts.down_proj], {"top_k": k})
    # the block takes its softmax in fp32 whatever the model's dtype: the weights agree to fp32 rounding
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())


# ------------------------------------------------------------------ 3. the builder
def test_mixtral_programs_hold_the_op_and_the_models_rope_theta(model):
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN)
    assert [p["name"] for p in progs] == ["mixtral-h256-l2-fp32-prefill8", "mixtral-h256-l2-fp32-step1"]
    moes = [n for n in progs[1]["nodes"] if n["op"] == "moe"]
    assert len(moes) == 2 and all(n["attrs"] == {"top_k": 2} for n in moes)
    assert not any(n["op"] in ("silu", "mul") for n in progs[1]["nodes"])
    ps = PG.parse_variants(progs, w, gpu=True)
    cos = ps[0].tensors("cpu")["rope.cos"].numpy()
    assert model.config.rope_parameters["rope_theta"] == 1e6 and not hasattr(model.config, "rope_theta")
    assert np.array_equal(cos, rope_tables(MAX_LEN, 128, 1e6)[0]) and not np.array_equal(cos, rope_tables(MAX_LEN, 128, 1e4)[0])


def test_builder_refusals(model):
    def build(m=model, max_len=MAX_LEN, **kw):
        return llama_decode_programs(m, PROMPT_LEN, max_len, **kw)

    with pytest.raises(ValueError, match="weights='int8' is not taken"):
        build(weights="int8")
    with pytest.raises(ValueError, match="dtype='bf16' is not taken"):
        build(dtype="bf16")
    A, B = np.zeros((4, 96), np.float32), np.zeros((256, 4), np.float32)
    with pytest.raises(ValueError, match="q / k / v / o only"):
        build(adapters=[{"model.layers.0.mlp.down_proj": (A, B, 1.0)}])
    windowed = mixtral_model(mixtral_config(sliding_window=MAX_LEN - 1), MODEL_SEED)
    with pytest.raises(ValueError, match="sliding_window = 47 is set and smaller than max_len = 48"):
        build(windowed)
    build(windowed, max_len=MAX_LEN - 1)   # a window that never slides is no refusal
    wide = mixtral_model(mixtral_config(num_hidden_layers=1, intermediate_size=4100, vocab_size=32), MODEL_SEED)
    with pytest.raises(ValueError, match=r"batch \* K \* max\(H, I\) \* 4 = 65600 > 65536"):
        build(wide, speculate=4)
    build(wide, speculate=3)


LLAMA_SETS = {   # sha256 of json.dumps(programs, sort_keys=True) as the builder produced them before the dispatch
    "plain": (dict(), "e6f4d1d223b688cf989d9a7d0fa543da65342f30ffb7e58cb177d6e7ae69d17e"),
    "batch-extend-sampling-stopping": (dict(batch=2, extend=(4,), sampling=True, stopping=True),
                                       "06e0df85fdcb7f575416728192d7a5c2d701ca0ce387cf5af1187157a6a068b0"),
    "kvq8-speculate": (dict(kv="int8", speculate=4), "0df8bcdc0796b2651ea5dbfdd9bf6f23c7c0878c6e499b4bcc273dab0401e896"),
    "int8": (dict(weights="int8"), "f895d85b6e11cf566c9960f1e0d3367b591df63f315dcb08da51fe42529e7fab"),
    "bf16": (dict(dtype="bf16"), "b224160db818d5accef296b899b798861472d1c7b2c918a8e22eee83e86e202c"),
}


def _check_payload(prog: dict, w: bytes, sd: dict, rope_rows: int) -> int:
    """Every fp32 param the state dict or the rotary tables (theta 10000) name holds exactly their bytes."""
    cos, sin = rope_tables(rope_rows, 128, 10000.0)
    known = {**sd, "rope.cos": cos, "rope.sin": sin}
    n = 0
    for p in prog["params"]:
        if p["name"] in known and p["dtype"] == "fp32":
            assert w[p["offset"]:p["offset"] + p["nbytes"]] == np.ascontiguousarray(known[p["name"]], np.float32).tobytes(), p["name"]
            n += 1
    return n


def test_llama_programs_are_unchanged():
    m = llama_model(llama_config(False), 0)
    sd = {k: v.detach().float().numpy() for k, v in m.state_dict().items()}
    for name, (kw, pin) in LLAMA_SETS.items():
        progs, w = llama_decode_programs(m, 16, 64, **kw)
        assert hashlib.sha256(json.dumps(progs, sort_keys=True).encode()).hexdigest() == pin, name
        assert all(p["name"].startswith("llama-") for p in progs)
        assert _check_payload(progs[-1], w, sd, 64) >= (2 if kw.get("dtype") == "bf16" else 3), name
    prog, w = llama_program(m, 16)
    assert hashlib.sha256(json.dumps(prog, sort_keys=True).encode()).hexdigest() == \
        "a467d1cf562f8198b320a8865859a3b0f435636d29f92ff5fa0d945f67d891cd"
    assert _check_payload(prog, w, sd, 16) == len(prog["params"])


def test_static_estimate_counts_the_expert_weights_once():
    est = {}
    for E in (4, 8):
        m = mixtral_model(mixtral_config(num_local_experts=E), MODEL_SEED)
        progs, w = llama_decode_programs(m, PROMPT_LEN, MAX_LEN, extend=(16,))
        ps = PG.parse_variants(progs, w)
        est[E] = [(p.bytes_estimate, p.param_bytes) for p in ps]
        assert ps[0].param_bytes == len(w)
    per_expert = 2 * (256 + 2 * 96 * 256 + 256 * 96) * 4   # two layers' router row and expert tensors
    (pre4, step4, ext4), (pre8, step8, ext8) = est[4], est[8]
    for (e4, p4), (e8, p8) in ((pre4, pre8), (step4, step8)):   # 8 rows and 1: the kernels' transients hold no E
        assert p8 - p4 == 4 * per_expert and e8 - e4 == 4 * per_expert
    # 16 rows, more than the kernels take: of the dense path's transients only the gates and the routing
    # probabilities [rows, E] grow with E (twice: the graph's buffers and the solo run's); the weights count once
    assert ext8[1] - ext4[1] == 4 * per_expert
    assert 4 * per_expert <= ext8[0] - ext4[0] <= 4 * per_expert + 2 * 16 * 3 * 4 * 4


def test_training_tenants_refuse_a_moe_program():
    from nos_amd.podserver.training import parse_train_spec

    prog, w = _moe_program()
    with pytest.raises(ProgramError, match="moe node cannot be a training tenant"):
        parse_train_spec({"loss": "mse"}, PG.parse(prog, w))


# ------------------------------------------------------------------ 4. the CPU pod server
def _serve(tmp_path, name, progs, w):
    srv = PodServer(tmp_path / f"{name}.sock", device="cpu", lanes=2, memory_gb=40).start()
    c = PodClient(srv.path, connect_timeout_s=5)
    c.register(name, progs[0], w, memory_limit_gb=1, variants=progs[1:])
    return srv, c


def test_cpu_server_generates_mixtrals_tokens(model, reference, tmp_path):
    with torch.no_grad():
        hf = model.generate(torch.from_numpy(prompt()).long(), max_new_tokens=NEW, do_sample=False, pad_token_id=PAD)
    assert np.array_equal(hf[:, PROMPT_LEN:].numpy(), reference[:1])
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN)
    srv, c = _serve(tmp_path, "moe", progs, w)
    try:
        for loop in (True, False):
            ids, t = c.generate(prompt(), NEW, server_loop=loop)
            assert np.array_equal(ids, reference[:1]), loop
            assert t["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
        c.close()
    finally:
        srv.stop()


def test_cpu_server_batch_two_and_an_extend(model, reference, tmp_path):
    progs, w = llama_decode_programs(model, PROMPT_LEN - 3, MAX_LEN, batch=2, extend=(3,))
    srv, c = _serve(tmp_path, "moe-b2", progs, w)
    try:
        two = prompt(2)
        c.infer(two[:, :PROMPT_LEN - 3])
        outs, _ = c.infer(two[:, PROMPT_LEN - 3:], outputs=[1])   # the extend variant finishes the prompt
        toks = [outs[0].reshape(2, 1).astype(np.int32)]
        for _ in range(NEW - 1):
            outs, rep = c.infer(toks[-1], outputs=[1])
            toks.append(outs[0].reshape(2, 1).astype(np.int32))
        assert np.array_equal(np.concatenate(toks, 1), reference)
        assert rep["state"] == {"pos": [PROMPT_LEN + NEW - 1] * 2}
        c.close()
    finally:
        srv.stop()


def test_cpu_server_stopping(model, reference, tmp_path):
    eos = int(reference[0, NEW // 2])
    first = int(np.flatnonzero(reference[0] == eos)[0])
    with torch.no_grad():
        hf = model.generate(torch.from_numpy(prompt()).long(), max_new_tokens=NEW, do_sample=False, eos_token_id=eos,
                            pad_token_id=PAD)
    want = hf[:, PROMPT_LEN:].numpy()
    assert np.array_equal(want, reference[:1, :first + 1])
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, stopping=True)
    srv, c = _serve(tmp_path, "moe-stop", progs, w)
    try:
        for loop in (True, False):
            ids, _ = c.generate(prompt(), NEW, server_loop=loop, eos_token_id=eos, pad_token_id=PAD)
            assert np.array_equal(ids, want), loop
            c.reset()
        assert np.array_equal(c.generate(prompt(), NEW)[0], reference[:1])   # no stop ids: the plain tokens
        c.close()
    finally:
        srv.stop()


def test_cpu_server_speculation_yields_the_same_tokens(model, reference, tmp_path):
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, speculate=4)
    assert progs[-1]["name"] == "mixtral-h256-l2-fp32-spec-verify4"
    srv, c = _serve(tmp_path, "moe-spec", progs, w)
    try:
        plain, _ = c.generate(prompt(), NEW)
        c.reset()
        spec, t = c.generate(prompt(), NEW, speculate=True)
        assert np.array_equal(plain, reference[:1]) and np.array_equal(spec, plain)
        assert t["steps_run"] <= NEW - 1
        c.close()
    finally:
        srv.stop()


def make_qv_adapter(model, rank: int = 4, seed: int = 5) -> dict:
    rng = np.random.default_rng(seed)
    sd = model.state_dict()
    ad = {}
    for i in range(model.config.num_hidden_layers):
        for t in ("self_attn.q_proj", "self_attn.v_proj"):
            name = f"model.layers.{i}.{t}"
            o, k = sd[name + ".weight"].shape
            ad[name] = ((rng.standard_normal((rank, k)) / np.sqrt(k)).astype(np.float32),
                        (rng.standard_normal((o, rank)) * 0.05).astype(np.float32), 2.0)
    return ad


def test_cpu_server_q_and_v_adapter_matches_adapted_llama(model, reference, tmp_path):
    ad = make_qv_adapter(model)
    want = reference_run(adapted_llama(model, ad), prompt())
    assert not np.array_equal(want, reference[:1]), "the adapter leaves the base model's ids unchanged"
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, adapters=[ad])
    assert progs[1]["name"] == "mixtral-h256-l2-fp32-lora-step1"
    srv, c = _serve(tmp_path, "moe-lora", progs, w)
    try:
        assert np.array_equal(c.generate(prompt(), NEW, adapter=1)[0], want)
        c.reset()
        assert np.array_equal(c.generate(prompt(), NEW, adapter=0)[0], reference[:1])
        c.close()
    finally:
        srv.stop()
