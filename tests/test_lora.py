"""Multi-adapter LoRA decoder tenants (CPU): the ``lora`` op through validator,
eager reference, Llama builder and the CPU pod server.  One tenant holds the
base weights once and N adapters; every request names an adapter per row.
Everything is compared against ``adapted_llama`` (the HF model with the
adapter's unmerged low-rank branches), never against merged weights."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

from nos_amd.models.llama_program import (adapted_llama, dequantized_llama, llama_config, llama_decode_programs,
                                          llama_model)
from nos_amd.ops import tenant as T
from nos_amd.podserver import program as PG
from nos_amd.podserver.client import PodClient, PodServerError
from nos_amd.podserver.program import Builder, ProgramError
from nos_amd.podserver.server import PodServer

PROMPT_LEN, NEW, MAX_LEN = 16, 32, 64
PROMPT_SEED = 0   # chosen so every reference's top-2 gap clears 1e-4 at every step (asserted below)
RANK, ALPHA = 8, 16
TARGETS = ("self_attn.q_proj", "self_attn.v_proj", "mlp.down_proj")


def make_adapters(model, n: int = 3, targets=TARGETS, rank: int = RANK, seed: int = 10) -> list[dict]:
    """n random adapters on ``targets`` of every layer.  A trained adapter's B is no longer zero: B is
    drawn at the scale of the weight it joins, so that the delta moves the logits (the references
    below assert that it changes the generated ids)."""
    rng = np.random.default_rng(seed)
    sd = model.state_dict()
    out = []
    for _ in range(n):
        ad = {}
        for i in range(model.config.num_hidden_layers):
            for t in targets:
                name = f"model.layers.{i}.{t}"
                o, k = sd[name + ".weight"].shape
                A = (rng.standard_normal((rank, k)) / np.sqrt(k)).astype(np.float32)
                B = (rng.standard_normal((o, rank)) * 0.05).astype(np.float32)
                ad[name] = (A, B, ALPHA / rank)
        out.append(ad)
    return out


@pytest.fixture(scope="module")
def model():
    return llama_model(llama_config(False), 0)


@pytest.fixture(scope="module")
def adapters(model):
    return make_adapters(model)


@pytest.fixture(scope="module")
def tenant(model, adapters):
    return llama_decode_programs(model, PROMPT_LEN, MAX_LEN, adapters=adapters)


@pytest.fixture(scope="module")
def tenant_plain(model):
    return llama_decode_programs(model, PROMPT_LEN, MAX_LEN)


def prompt(rows: int = 1, seed: int = PROMPT_SEED) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 512, (rows, PROMPT_LEN)).astype(np.int32)


def greedy_ids_and_gap(m, ids: np.ndarray, new: int = NEW) -> tuple[np.ndarray, float]:
    """Greedy ids of ``m`` in fp64 for the one-row prompt ``ids``, and the smallest top-2 logit gap
    over the generated steps relative to the largest |logit|."""
    m64 = copy.deepcopy(m).double()
    seq = torch.from_numpy(ids.astype(np.int64))
    gap = float("inf")
    with torch.no_grad():
        for _ in range(new):
            logits = m64(seq).logits[0, -1]
            top = logits.topk(2)
            gap = min(gap, float((top.values[0] - top.values[1]) / logits.abs().max()))
            seq = torch.cat([seq, top.indices[:1].view(1, 1)], 1)
    return seq[:, ids.shape[1]:].numpy(), gap


@pytest.fixture(scope="module")
def reference(model, adapters):
    """[ids of the base model, ids under adapter 1, 2, 3] for ``prompt()``, each [1, NEW], from fp64
    runs of ``adapted_llama``; asserted: no near tie, and the adapters matter."""
    runs = [greedy_ids_and_gap(model, prompt())] + [greedy_ids_and_gap(adapted_llama(model, a), prompt())
                                                    for a in adapters]
    gap = min(g for _, g in runs)
    assert gap >= 1e-4, f"top-2 gap {gap}: pick another PROMPT_SEED (the test must not ride on a near tie)"
    ids = [r for r, _ in runs]
    assert all(not np.array_equal(ids[0], r) for r in ids[1:]), "an adapter leaves the base model's ids unchanged"
    assert any(not np.array_equal(ids[i], ids[j]) for i in range(1, 4) for j in range(i + 1, 4)), \
        "every adapter generates the same ids"
    return ids


# ------------------------------------------------------------------ 1. the validator
def _lora_program(batch: int = 2, s: int = 3, k: int = 32, n_out: int = 24, n: int = 3, r: int = 8,
                  x_dtype: str = "fp32"):
    rng = np.random.default_rng(1)
    b = Builder("lora")
    x = b.input("x", [batch, s, k], "fp32")
    if x_dtype != "fp32":
        x = b.op("cast", x, dtype=x_dtype)
    sel = b.adapter_state(batch)
    w = b.param("w", rng.standard_normal((n_out, k)), x_dtype)
    A = b.param("A", rng.standard_normal((n, r, k)))
    B = b.param("B", rng.standard_normal((n, n_out, r)))
    y = b.op("add", b.op("linear", x, w), b.op("lora", x, A, B, sel, out="delta"), out="y")
    return b.build([y])


def test_validator_accepts_a_well_formed_lora_program():
    prog, w = _lora_program()
    p = PG.parse(prog, w, gpu=True)
    assert p.values["delta"].shape == (2, 3, 24) and p.values["delta"].dtype == "fp32"
    assert p.adapter_state == "adapter" and p.adapters == 3
    assert p.state["adapter"].shape == (2,) and p.state["adapter"].dtype == "i32"
    assert "lora" in PG.OPS and "lora" in PG.NEVER_FOLD and "lora_shrink" in PG.NATIVE_KINDS
    assert p.foldable() == set()


def _param(p, name):
    return next(q for q in p["params"] if q["name"] == name)


def _node(p, op):
    return next(n for n in p["nodes"] if n["op"] == op)


def _sel_is_a_node_value(p):
    p["nodes"].insert(0, {"op": "argmax", "inputs": ["x"], "output": "picked", "attrs": {}})
    _node(p, "lora")["inputs"][3] = "picked"


def _sel_wrong_shape(p):
    p["state"][0].update(shape=[3])


def _sel_wrong_dtype(p):
    p["state"][0].update(dtype="fp32")


def _reshape_param(name, shape):
    def mutate(p):
        q = _param(p, name)
        assert int(np.prod(shape)) * 4 == q["nbytes"]
        q.update(shape=shape)
    return mutate


def _two_adapter_states(p):
    p["state"].append({"name": "adapter2", "shape": [2], "dtype": "i32"})
    p["nodes"].insert(-1, {"op": "lora", "inputs": ["x", "A", "B", "adapter2"], "output": "delta2", "attrs": {}})


def _adapter_state_as_output(p):
    p["outputs"].append("adapter")


def _adapter_is_also_the_sampling_state(p):
    p["state"][0].update(shape=[4])
    p["inputs"][0].update(shape=[4, 3, 32])
    p["state"].append({"name": "pos", "shape": [12], "dtype": "i32"})
    p["nodes"].append({"op": "sample", "inputs": ["y", "adapter", "pos"], "output": "ids", "attrs": {}})


@pytest.mark.parametrize("mutate, match", [
    (_sel_is_a_node_value, "sel must be a state"),
    (_sel_wrong_shape, r"sel must be an i32 \[2\] state"),
    (_sel_wrong_dtype, r"sel must be an i32 \[2\] state"),
    (_reshape_param("A", [2, 12, 32]), "same number of adapters n"),          # n: 2 against B's 3
    (_reshape_param("A", [3, 4, 64]), "share the rank R"),                   # R: 4 against B's 8
    (_reshape_param("B", [3, 48, 4]), "share the rank R"),
    (_reshape_param("A", [3, 16, 16]), "share the rank R"),
    (_reshape_param("A", [6, 8, 16]), "same number of adapters n"),
    (_two_adapter_states, "one adapter state"),
    (_adapter_state_as_output, "adapter state 'adapter' cannot be an output"),
    (_adapter_is_also_the_sampling_state, "control states of different kinds must be different states"),
])
def test_validator_refusals(mutate, match):
    prog, w = _lora_program()
    prog = copy.deepcopy(prog)
    mutate(prog)
    with pytest.raises(ProgramError, match=match):
        PG.parse(prog, w)


def test_validator_refuses_a_mismatched_k_and_a_bf16_x():
    prog, w = _lora_program()
    prog = copy.deepcopy(prog)
    _param(prog, "A").update(shape=[3, 16, 16])
    _param(prog, "B").update(shape=[3, 12, 16])
    with pytest.raises(ProgramError, match=r"must have x's K = 32"):
        PG.parse(prog, w)
    prog, w = _lora_program(x_dtype="bf16")
    with pytest.raises(ProgramError, match="x must be fp32.*bf16"):
        PG.parse(prog, w)


def test_validator_checks_the_kernels_rank_on_the_gpu():
    prog, w = _lora_program(r=6)
    PG.parse(prog, w)
    with pytest.raises(ProgramError, match="R % 4 == 0"):
        PG.parse(prog, w, gpu=True)


# ------------------------------------------------------------------ 2. the eager reference
def test_reference_is_the_literal_per_row_loop_bit_for_bit():
    rng = torch.Generator().manual_seed(3)
    n, R, K, N = 3, 8, 32, 24
    x = torch.randn(6, 5, K, generator=rng)
    A, B = torch.randn(n, R, K, generator=rng), torch.randn(n, N, R, generator=rng)
    sel = torch.tensor([0, 1, 3, n + 1, -1, 2], dtype=torch.int32)
    got = T.lora_ref(x, A, B, sel)
    assert got.shape == (6, 5, N) and got.dtype == torch.float32
    for b, a in enumerate(sel.tolist()):
        want = (x[b] @ A[a - 1].T) @ B[a - 1].T if 1 <= a <= n else torch.zeros(5, N)
        assert torch.equal(got[b], want), (b, a)
    assert not got[1].eq(0).all() and got[0].eq(0).all() and got[3].eq(0).all() and got[4].eq(0).all()
    # the program's reference runs the same definition
    prog, w = _lora_program(batch=6, s=5, k=K, n_out=N, n=n, r=R)
    p = PG.parse(prog, w)
    ps = p.tensors("cpu")
    st = p.state_tensors("cpu")
    st["adapter"].copy_(sel)
    y, = p.reference(x, ps, st)
    assert torch.equal(y, torch.nn.functional.linear(x, ps["w"]) + T.lora_ref(x, ps["A"], ps["B"], sel))


def test_shrink_and_expand_references_compose_to_the_op():
    rng = torch.Generator().manual_seed(4)
    n, R, K, N = 3, 12, 48, 20
    x = torch.randn(2, 4, K, generator=rng, dtype=torch.float64)
    A, B = (torch.randn(n, R, K, generator=rng, dtype=torch.float64),
            torch.randn(n, N, R, generator=rng, dtype=torch.float64))
    sel = torch.tensor([2, 0], dtype=torch.int32)
    t = T.lora_shrink_ref(x.reshape(8, K), A, sel, rows_per_seq=4, dtype=torch.float64)
    d = T.lora_expand_ref(t, B, sel, rows_per_seq=4, dtype=torch.float64)
    assert torch.allclose(d.reshape(2, 4, N), T.lora_ref(x, A, B, sel), rtol=1e-12, atol=1e-12)
    assert t[4:].eq(0).all() and d[4:].eq(0).all()


# ------------------------------------------------------------------ 3. the Llama builder
def _with(ad: dict, **changes) -> dict:
    out = dict(ad)
    out.update(changes)
    return out


def test_builder_refusals(model, adapters):
    name = "model.layers.0.self_attn.q_proj"
    A, B, sc = adapters[0][name]
    wide = np.zeros((16, A.shape[1]), np.float32), np.zeros((B.shape[0], 16), np.float32), sc
    with pytest.raises(ValueError, match="share one rank"):
        llama_decode_programs(model, PROMPT_LEN, MAX_LEN, adapters=[adapters[0], _with(adapters[1], **{name: wide})])
    fewer = {k: v for k, v in adapters[1].items() if k != name}
    with pytest.raises(ValueError, match="share one target set"):
        llama_decode_programs(model, PROMPT_LEN, MAX_LEN, adapters=[adapters[0], fewer])
    big = make_adapters(model, 1, ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), rank=24)
    with pytest.raises(ValueError, match="stacked rank R = 24 x 3 = 72"):
        llama_decode_programs(model, PROMPT_LEN, MAX_LEN, adapters=big)
    odd = make_adapters(model, 1, ("self_attn.o_proj",), rank=6)
    with pytest.raises(ValueError, match="multiple of 4"):
        llama_decode_programs(model, PROMPT_LEN, MAX_LEN, adapters=odd)
    with pytest.raises(ValueError, match="dtype must be 'fp32'"):
        llama_decode_programs(model, PROMPT_LEN, MAX_LEN, dtype="bf16", adapters=adapters)
    with pytest.raises(ValueError, match="unknown module name 'model.layers.0.self_attn.w_proj'"):
        llama_decode_programs(model, PROMPT_LEN, MAX_LEN,
                              adapters=[_with(adapters[0], **{"model.layers.0.self_attn.w_proj": (A, B, sc)})])
    with pytest.raises(ValueError, match="unknown module name 'model.layers.2.mlp.up_proj'"):   # the model has 2 layers
        llama_decode_programs(model, PROMPT_LEN, MAX_LEN,
                              adapters=[_with(adapters[0], **{"model.layers.2.mlp.up_proj": (A, B, sc)})])


def test_payload_is_the_plain_tenants_plus_the_adapters(model, adapters, tenant, tenant_plain):
    progs, w = tenant
    plain, wp = tenant_plain
    cfg = model.config
    d, hd = cfg.hidden_size, cfg.hidden_size // cfg.num_attention_heads
    qkv = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * hd
    # per layer: q + v stacked on the merged q / k / v columns (R = 2 r; k's rows and the off-diagonal
    # blocks are stored zeros), down on its own
    per_layer = 3 * (2 * RANK * d + qkv * 2 * RANK) + 3 * (RANK * cfg.intermediate_size + d * RANK)
    assert len(w) == len(wp) + 4 * cfg.num_hidden_layers * per_layer
    parsed = PG.parse_variants(progs, w)
    assert len(parsed) == 2 and all(p.adapter_state == "adapter" and p.adapters == 3 for p in parsed)
    assert all(p.param_layout == parsed[0].param_layout for p in parsed)
    lora = {k: v for k, v in parsed[0].params.items() if ".lora_" in k}
    assert sum(v.nbytes for v in lora.values()) == 4 * cfg.num_hidden_layers * per_layer
    assert parsed[0].param_bytes - sum(v.nbytes for v in lora.values()) == PG.parse(plain[0], wp).param_bytes
    # the estimate charges A and B at their bytes (they are params), and a decode step's t per lora node
    assert parsed[1].bytes_estimate >= parsed[1].param_bytes + parsed[1].state_bytes


def test_program_reference_matches_adapted_llama(model, adapters, tenant):
    """The prefill program's eager reference against the HF model with the adapter's branches, in
    fp32 arithmetic both (summation orders differ: 1e-4 of the logits' scale)."""
    progs, w = tenant
    p = PG.parse(progs[0], w)
    x = torch.from_numpy(prompt())
    for a in (0, 2):
        st = p.state_tensors("cpu")
        st["adapter"].fill_(a)
        logits = p.reference(x, state=st)[0]
        m = model if a == 0 else adapted_llama(model, adapters[a - 1])
        with torch.no_grad():
            want = m(x.long()).logits[:, -1:]
        assert (logits - want).abs().max() <= 1e-4 * want.abs().max()


# ------------------------------------------------------------------ 4. the CPU pod server
def _serve(tmp_path, name, progs, w, memory_gb=1):
    srv = PodServer(tmp_path / f"{name}.sock", device="cpu", lanes=2, memory_gb=40).start()
    c = PodClient(srv.path, connect_timeout_s=5)
    c.register(name, progs[0], w, memory_limit_gb=memory_gb, variants=progs[1:])
    return srv, c


def test_cpu_server_generates_each_adapters_tokens(reference, tenant, tenant_plain, tmp_path):
    progs, w = tenant
    srv, c = _serve(tmp_path, "lora", progs, w)
    try:
        for a in range(4):
            x, tx = c.generate(prompt(), NEW, server_loop=True, adapter=a)
            y, ty = c.generate(prompt(), NEW, server_loop=False, adapter=a)
            assert np.array_equal(x, reference[a]) and np.array_equal(y, reference[a]), a
            assert tx["state"] == ty["state"] == {"pos": [PROMPT_LEN + NEW - 1]}   # the adapter state is not replied
        base, _ = c.generate(prompt(), NEW)          # no field: the base model, whatever ran before
        assert np.array_equal(base, reference[0])
        c2 = PodClient(srv.path, connect_timeout_s=5)
        c2.register("plain", tenant_plain[0][0], tenant_plain[1], memory_limit_gb=1, variants=tenant_plain[0][1:])
        assert np.array_equal(c2.generate(prompt(), NEW)[0], base)
        c2.close()
        c.close()
    finally:
        srv.stop()


def test_batch_rows_take_their_own_adapters(model, adapters, reference, tmp_path):
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, batch=2, adapters=adapters)
    srv, c = _serve(tmp_path, "lora-b2", progs, w)
    try:
        two = np.repeat(prompt(), 2, axis=0)
        for pair in ([2, 0], [1, 3]):
            c.reset()
            for loop in (True, False):
                got, _ = c.generate(two, NEW, server_loop=loop, adapter=pair)
                assert np.array_equal(got[0:1], reference[pair[0]]) and np.array_equal(got[1:2], reference[pair[1]]), pair
        c.close()
    finally:
        srv.stop()


def test_bad_adapter_fields_are_refused_and_leave_the_positions(tenant, tenant_plain, tmp_path):
    progs, w = tenant
    srv, c = _serve(tmp_path, "lora", progs, w)
    try:
        _, rep = c.infer(prompt(), outputs=[1], adapter=1)
        assert rep["state"] == {"pos": [PROMPT_LEN]}
        for bad, match in ((4, r"ids must lie in \[0, 3\]"), (-1, r"ids must lie in \[0, 3\]"),
                           ([1, 2], "a list of 1 ints"), ([1.5], "a list of 1 ints"), ("1", "a list of 1 ints")):
            with pytest.raises(PodServerError, match=match):
                c.infer(np.zeros((1, 1), np.int32), outputs=[1], adapter=bad)
            with pytest.raises(PodServerError, match=match):
                c._call({"op": "generate", "steps": 2, "output": 1, "shape": [1, 1], "dtype": "i32", "adapter": bad},
                        np.zeros((1, 1), np.int32).tobytes())
        assert c.infer(np.zeros((1, 1), np.int32), outputs=[1], adapter=3)[1]["state"] == {"pos": [PROMPT_LEN + 1]}
        c2 = PodClient(srv.path, connect_timeout_s=5)
        c2.register("plain", tenant_plain[0][0], tenant_plain[1], memory_limit_gb=1, variants=tenant_plain[0][1:])
        c2.infer(prompt(), outputs=[1])
        with pytest.raises(PodServerError, match="hold no adapters"):
            c2.infer(np.zeros((1, 1), np.int32), outputs=[1], adapter=0)
        assert c2.infer(np.zeros((1, 1), np.int32), outputs=[1])[1]["state"] == {"pos": [PROMPT_LEN + 1]}
        c2.close()
        c.close()
    finally:
        srv.stop()


# ------------------------------------------------------------------ 5. combinations
def test_int8_weights_with_adapters_match_the_adapted_dequantized_model(model, adapters, tmp_path):
    deq = dequantized_llama(model)
    want, gap = greedy_ids_and_gap(adapted_llama(deq, adapters[1]), prompt())
    assert gap >= 1e-4, gap
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, weights="int8", adapters=adapters)
    srv, c = _serve(tmp_path, "lora-q8", progs, w)
    try:
        assert np.array_equal(c.generate(prompt(), NEW, adapter=2)[0], want)
        c.close()
    finally:
        srv.stop()


def test_stopping_with_zero_control_words_is_the_adapter_tenants_tokens(model, adapters, reference, tmp_path):
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, stopping=True, adapters=adapters)
    srv, c = _serve(tmp_path, "lora-stop", progs, w)
    try:
        assert np.array_equal(c.generate(prompt(), NEW, adapter=3)[0], reference[3])
        c.close()
    finally:
        srv.stop()


def test_speculation_yields_the_same_adapter_tokens(model, adapters, reference, tmp_path):
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, speculate=4, adapters=adapters)
    srv, c = _serve(tmp_path, "lora-spec", progs, w)
    try:
        plain, _ = c.generate(prompt(), NEW, adapter=1)
        spec, t = c.generate(prompt(), NEW, adapter=1, speculate=True)
        assert np.array_equal(spec, plain) and np.array_equal(plain, reference[1])
        assert t["steps_run"] < NEW - 1 or t["n_acc"].max() == 1   # accepted drafts: fewer steps than tokens
        c.close()
    finally:
        srv.stop()
