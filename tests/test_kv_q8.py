"""Int8 K / V caches for decoder tenants on the CPU: the validator's rules for
i8 cache states and their scales states, the eager reference ops, a whole
tenant against the HF model run with ``kv_q8_roundtrip_cache()``, the paths
that must compute one function, the memory estimate and the builder argument.

A cache row (one (sequence, position, KV head) vector) is stored as int8 values
plus one fp32 scale by ``quantize_rows_q8``'s rule on the row in fp32; what the
cache holds is ``float(q) * scale`` and every attention is exact fp32 arithmetic
on those values."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

from nos_amd.models.llama_program import (kv_q8_roundtrip_cache, llama_config, llama_decode_programs, llama_model)
from nos_amd.podserver import program as PG
from nos_amd.podserver.program import Builder, dequantize_rows_q8, quantize_rows_q8
from nos_amd.podserver.program.reference import kv_write_ref, sdpa_cache_ref

B, L, HKV, D, H = 2, 16, 2, 64, 4


# ------------------------------------------------------------------ validator
def _prog(kdt="i8", kscales=True, sc_shape=(B, L, HKV), sc_dt="fp32", xdt="fp32", vs="vs", outputs=None, extra=None,
          read_dead=False):
    """One layer: kv_write K and V, then sdpa_cache; ``extra(b, names)`` adds nodes before the build."""
    b = Builder("kvq8")
    x = b.input("x", [B, 2, (H + 2 * HKV) * D], "fp32")
    if xdt != "fp32":
        x = b.op("cast", x, dtype=xdt)
    b.state("pos", [B], "i32")
    kc, vc = b.state("kc", [B, L, HKV, D], kdt), b.state("vc", [B, L, HKV, D], kdt)
    b.state("ks", list(sc_shape), sc_dt)
    b.state("vs", [B, L, HKV], "fp32")
    q = b.op("reshape", b.op("slice", x, dim=-1, start=0, end=H * D), shape=[B, 2, H, D])
    k = b.op("reshape", b.op("slice", x, dim=-1, start=H * D, end=(H + HKV) * D), shape=[B, 2, HKV, D])
    v = b.op("reshape", b.op("slice", x, dim=-1, start=(H + HKV) * D, end=(H + 2 * HKV) * D), shape=[B, 2, HKV, D])
    kc1 = b.op("kv_write", kc, k, "pos", *(["ks"] if kscales else []))
    vc1 = b.op("kv_write", vc, v, "pos", *([vs] if kscales else []))
    o = b.op("sdpa_cache", q, kc if read_dead else kc1, vc1, "pos", *(["ks", vs] if kscales else []))
    names = dict(q=q, k=k, v=v, kc=kc1, vc=vc1, o=o)
    if extra is not None:
        o = extra(b, names) or o
    return b.build(outputs or [o])


def test_validator_takes_i8_caches_with_their_scales():
    p = PG.parse(*_prog())
    assert p.state["kc"].dtype == "i8" and p.state["ks"].shape == (B, L, HKV)
    assert p.values[p.outputs[0]].shape == (B, 2, H, D) and p.values[p.outputs[0]].dtype == "fp32"
    PG.parse(*_prog(kdt="fp32", kscales=False))      # the 3- and 4-input forms are as they were


@pytest.mark.parametrize("kw, msg", [
    (dict(extra=lambda b, n: b.op("add", n["kc"], n["kc"])), "i8 state; only kv_write and sdpa_cache"),
    (dict(extra=lambda b, n: b.op("kv_write", n["vc"], n["v"], "pos", n["kc"])), "i8 state; only kv_write and sdpa_cache"),
    (dict(kscales=False), "an i8 cache needs its scales state"),
    (dict(kdt="fp32"), "cache takes no scales"),
    (dict(kdt="bf16", xdt="bf16"), "cache takes no scales"),
    (dict(sc_shape=(B, L, HKV, 1)), r"scales of an i8 cache must be an fp32 \[2, 16, 2\] state"),
    (dict(sc_shape=(B, L)), r"scales of an i8 cache must be an fp32 \[2, 16, 2\] state"),
    (dict(sc_dt="bf16"), r"scales of an i8 cache must be an fp32 \[2, 16, 2\] state"),
    (dict(sc_dt="i32"), r"scales of an i8 cache must be an fp32 \[2, 16, 2\] state"),
    (dict(vs="ks"), "it cannot also hold the scales of"),
    (dict(outputs=["ks"]), "scales state 'ks' of the i8 cache 'kc' cannot be an output"),
    (dict(extra=lambda b, n: b.op("add", b.op("reshape", "ks", shape=[B, L, HKV]), "vs")), "a scales state is named only"),
    (dict(xdt="bf16"), "x must be .* fp32"),
    (dict(read_dead=True), "was updated in place before this node"),
    (dict(outputs=["kc"]), "cannot be an output"),
])
def test_validator_refusals(kw, msg):
    with pytest.raises(PG.ProgramError, match=msg):
        PG.parse(*_prog(**kw))


def test_validator_refuses_bf16_q_a_second_scales_state_and_scales_as_x():
    def bf16_q(b, n):   # the attention of i8 caches takes an fp32 q
        return b.op("sdpa_cache", b.op("cast", n["q"], dtype="bf16"), n["kc"], n["vc"], "pos", "ks", "vs")

    with pytest.raises(PG.ProgramError, match="q must be fp32 over i8 caches"):
        PG.parse(*_prog(extra=bf16_q))

    def other_scales(b, n):   # the pairing is fixed for the program: kc keeps its scales in ks
        b.state("ks2", [B, L, HKV], "fp32")
        return b.op("sdpa_cache", n["q"], n["kc"], n["vc"], "pos", "ks2", "vs")

    with pytest.raises(PG.ProgramError, match="keeps its scales in 'ks', not in 'ks2'"):
        PG.parse(*_prog(extra=other_scales))
    with pytest.raises(PG.ProgramError, match="input dtype must be one of"):     # i8 is no input dtype either
        p, w = _prog()
        p["inputs"][0]["dtype"] = "i8"
        PG.parse(p, w)
    with pytest.raises(PG.ProgramError, match="state dtype i8 is a quantized K / V cache's"):     # an unused i8 state
        PG.parse(*_prog(extra=lambda b, n: b.state("spare", [B, L, HKV, D], "i8") and None))
    with pytest.raises(PG.ProgramError, match="4 inputs"):
        PG.parse(*_prog(extra=lambda b, n: b.op("sdpa_cache", n["q"], n["kc"], n["vc"], "pos", "ks")))


# ------------------------------------------------------------------ reference ops
def test_kv_write_ref_quantizes_rows_by_the_weights_rule():
    g = torch.Generator().manual_seed(0)
    S = 5
    x = torch.randn(3, S, HKV, D, generator=g) * torch.logspace(-3, 3, 3 * S * HKV).view(3, S, HKV, 1)
    x[1, 2, 1] = 0                                   # an all-zero row: scale 1
    pos = torch.tensor([0, L - 2, -3], dtype=torch.int32)     # rows past L and negative positions are dropped
    cache = torch.full((3, L, HKV, D), 77, dtype=torch.int8)
    scales = torch.full((3, L, HKV), -5.0)
    out = kv_write_ref(cache, x, pos, scales)
    assert out is cache
    q, s = quantize_rows_q8(x.reshape(-1, D).numpy())
    q, s = torch.from_numpy(q).view(3, S, HKV, D), torch.from_numpy(s).view(3, S, HKV)
    assert torch.equal(cache[0, :S], q[0]) and torch.equal(scales[0, :S], s[0])
    assert torch.equal(cache[1, L - 2:], q[1, :2]) and torch.equal(scales[1, L - 2:], s[1, :2])
    assert float(s[1, 2, 1]) == 1.0 and not q[1, 2, 1].any()
    untouched = torch.ones(3, L, dtype=torch.bool)
    untouched[0, :S] = False
    untouched[1, L - 2:] = False
    assert bool((cache[untouched] == 77).all()) and bool((scales[untouched] == -5.0).all())
    deq = torch.from_numpy(dequantize_rows_q8(q.reshape(-1, D).numpy(), s.reshape(-1).numpy())).view(3, S, HKV, D)
    assert bool(((deq - x).abs() <= s[..., None] / 2 * (1 + 2.0 ** -20)).all())
    # fp64 rows are quantized in fp32 all the same
    c2, s2 = torch.zeros_like(cache), torch.zeros_like(scales)
    kv_write_ref(c2, x.double(), pos, s2)
    assert torch.equal(c2[0, :S], q[0]) and torch.equal(s2[0, :S], s[0])
    with pytest.raises(ValueError):
        kv_write_ref(cache, x, pos)
    with pytest.raises(ValueError):
        kv_write_ref(cache.float(), x, pos, scales)


def test_sdpa_cache_ref_attends_the_dequantized_rows():
    g = torch.Generator().manual_seed(1)
    kc = torch.randint(-127, 128, (B, L, HKV, D), generator=g, dtype=torch.int8)
    vc = torch.randint(-127, 128, (B, L, HKV, D), generator=g, dtype=torch.int8)
    ks, vs = torch.rand(B, L, HKV, generator=g) + 0.1, torch.rand(B, L, HKV, generator=g) + 0.1
    q = torch.randn(B, 3, H, D, generator=g) / 50
    pos = torch.tensor([0, 9], dtype=torch.int32)
    kd, vd = kc.float() * ks[..., None], vc.float() * vs[..., None]
    assert torch.equal(sdpa_cache_ref(q, kc, vc, pos, None, ks, vs), sdpa_cache_ref(q, kd, vd, pos))
    o64 = sdpa_cache_ref(q.double(), kc, vc, pos, None, ks, vs)
    assert o64.dtype == torch.float64 and torch.equal(o64, sdpa_cache_ref(q.double(), kd.double(), vd.double(), pos))
    with pytest.raises(ValueError):
        sdpa_cache_ref(q, kc, vc, pos)


# ------------------------------------------------------------------ a whole tenant
SEED = 0     # model and prompt; the bars below were checked to hold for seeds 0 .. 3 on the CPU
MAX_LEN = 32


@pytest.fixture(scope="module")
def model():
    return llama_model(llama_config(False), SEED)


def _ids(n):
    return torch.randint(0, 512, (1, n), generator=torch.Generator().manual_seed(SEED), dtype=torch.int32)


def _compiled(model, prompt_len, extend=(), **kw):
    progs, w = llama_decode_programs(model, prompt_len, MAX_LEN, kv="int8", extend=extend, **kw)
    ps = PG.parse_variants(progs, w)
    params, state = ps[0].tensors("cpu"), ps[0].state_tensors("cpu")
    return [p.compile("cpu", params=params, state=state) for p in ps], state, ps


def _hf_steps(m, ids, cache):
    out = []
    with torch.no_grad():
        r = m(ids[:, :8].long(), past_key_values=cache, use_cache=True)
        out.append(r.logits[:, -1:])
        for t in range(8, ids.shape[1]):
            r = m(ids[:, t:t + 1].long(), past_key_values=r.past_key_values, use_cache=True)
            out.append(r.logits[:, -1:])
    return torch.cat(out, 1)


def test_int8_kv_tenant_is_the_hf_model_with_the_roundtrip_cache(model):
    """Prefill 8 + 3 steps, the four logit rows against the HF model in fp64 run with
    ``kv_q8_roundtrip_cache()``: e <= max(4 e32, 1e-5), e32 the same HF run in fp32.
    Quantization is discontinuous (a value at a rounding boundary may fall to the
    other side in another summation order), so the seed matters: checked on the CPU
    for seeds 0 .. 3, e = 2.1e-7 .. 3.3e-7 against e32 = 2.1e-7 .. 3.1e-7; seed 0 is used."""
    ids = _ids(11)
    (pre, step), state, ps = _compiled(model, 8)
    assert state["kc0"].dtype == torch.int8 and state["ks0"].dtype == torch.float32
    assert state["ks0"].shape == (1, MAX_LEN, 1) and step.stats["kv_q8_caches"] == 4
    with torch.no_grad():
        got = [pre(ids[:, :8])[0]] + [step(ids[:, t:t + 1])[0] for t in range(8, 11)]
    got = torch.cat(got, 1)
    assert state["pos"].tolist() == [11]
    r32 = _hf_steps(model, ids, kv_q8_roundtrip_cache())
    r64 = _hf_steps(copy.deepcopy(model).double(), ids, kv_q8_roundtrip_cache())
    scale = float(r64.abs().max())
    e = float((got.double() - r64).abs().max()) / scale
    e32 = float((r32.double() - r64).abs().max()) / scale
    print(f"e = {e:.3g}, e32 = {e32:.3g}")
    assert e <= max(4 * e32, 1e-5), (e, e32)
    # the eager, unfused reference computes the same, from the same (int8) state
    rstate = {k: t.clone().zero_() for k, t in state.items()}
    ref = [ps[0].reference(ids[:, :8], state=rstate)[0]] + [ps[1].reference(ids[:, t:t + 1], state=rstate)[0]
                                                              for t in range(8, 11)]
    torch.testing.assert_close(got, torch.cat(ref, 1), rtol=1e-5, atol=1e-5)
    assert rstate["kc0"].dtype == torch.int8 and torch.equal(rstate["kc0"], state["kc0"])
    # the caches hold the quantized rows of the HF model's K and V (what an unwritten row holds is zero)
    assert not state["kc0"][0, 11:].any() and not state["ks0"][0, 11:].any() and bool(state["kc0"][0, :11].any())


def test_one_function_across_prefill_extend_and_steps(model):
    """prefill(8) + extend(4), prefill(8) + four one-token steps and prefill(12) (which
    hands the dequantized rows to the flash attention) compute one function: the last
    logits agree to fp32 round-off and the caches' bytes and scales are equal (seed 0:
    no K value sits at a rounding boundary between the paths; asserted)."""
    ids = _ids(12)
    (pre, step, ext), sa, _ = _compiled(model, 8, extend=(4,))
    with torch.no_grad():
        pre(ids[:, :8])
        a = ext(ids[:, 8:])[0]
    (pre_b, step_b, _), sb, _ = _compiled(model, 8, extend=(4,))
    with torch.no_grad():
        pre_b(ids[:, :8])
        for t in range(8, 12):
            b_ = step_b(ids[:, t:t + 1])[0]
    (pre_c, _), sc, _ = _compiled(model, 12)
    assert pre_c.stats["static_positions"] == 3 * model.config.num_hidden_layers
    assert sum(1 for s in pre_c.steps if s.kind == "sdpa") == model.config.num_hidden_layers
    assert all(s.kind != "sdpa_cache" for s in pre_c.steps)
    with torch.no_grad():
        c = pre_c(ids)[0]
    assert sa["pos"].tolist() == sb["pos"].tolist() == sc["pos"].tolist() == [12]
    torch.testing.assert_close(a, b_, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(a, c, rtol=1e-5, atol=1e-5)
    # the projections of 1, 4 and 12 rows sum in different orders, so a row's maximum -- its scale -- may
    # differ in the last bits between the paths; the int8 values do not (no value at a rounding boundary)
    for k in sa:
        for other in (sb, sc):
            if sa[k].dtype == torch.float32:
                torch.testing.assert_close(sa[k], other[k], rtol=1e-5, atol=0)
            else:
                assert torch.equal(sa[k], other[k]), k


def test_estimate_charges_an_i8_cache_its_bytes_and_scales(model):
    q8, w8 = llama_decode_programs(model, 8, MAX_LEN, kv="int8")
    f32, w32 = llama_decode_programs(model, 8, MAX_LEN)
    assert w8 == w32                                  # the weights do not change
    p8, p32 = PG.parse_variants(q8, w8), PG.parse_variants(f32, w32)
    caches = {k: v for k, v in p8[1].state.items() if v.dtype == "i8"}
    assert len(caches) == 2 * model.config.num_hidden_layers
    scales = sum(p8[1].state[k.replace("c", "s")].numel * 4 for k in caches)
    saved = sum(4 * v.numel for v in caches.values()) - (sum(v.numel for v in caches.values()) + scales)
    assert saved > 0 and p8[1].state_bytes == p32[1].state_bytes - saved
    assert p8[1].bytes_estimate == p32[1].bytes_estimate - saved            # a step: the states and nothing else
    # the prefill hands K and V over dequantized: at most two fp32 [B, S, Hkv, D] transients (times the
    # estimate's two graphs), and only if they sit at the peak
    deq = 2 * 8 * model.config.num_key_value_heads * 128 * 4
    assert p32[0].bytes_estimate - saved <= p8[0].bytes_estimate <= p32[0].bytes_estimate - saved + 2 * deq


def test_builder_argument(model):
    with pytest.raises(ValueError, match="dtype must be 'fp32'"):
        llama_decode_programs(model, 8, MAX_LEN, dtype="bf16", kv="int8")
    with pytest.raises(ValueError, match="kv must be"):
        llama_decode_programs(model, 8, MAX_LEN, kv="int4")
    assert llama_decode_programs(model, 8, MAX_LEN, kv="fp32") == llama_decode_programs(model, 8, MAX_LEN)
    progs, _ = llama_decode_programs(model, 8, MAX_LEN, kv="int8", weights="int8", sampling=True, extend=(4,), batch=2)
    for p in PG.parse_variants(progs, _):
        assert p.state["kc1"].dtype == "i8" and p.state["vs1"].shape == (2, MAX_LEN, 1) and p.sampling_state
        assert [len(n.inputs) for n in p.nodes if n.op == "kv_write"] == [4] * 4
        assert [len(n.inputs) for n in p.nodes if n.op == "sdpa_cache"] == [6] * 2


def test_roundtrip_cache_quantizes_per_token_and_head():
    g = torch.Generator().manual_seed(2)
    cache = kv_q8_roundtrip_cache()
    k, v = torch.randn(1, 2, 3, 64, generator=g).double(), torch.randn(1, 2, 3, 64, generator=g)
    ko, vo = cache.update(k, v, 0)
    want = torch.from_numpy(dequantize_rows_q8(*quantize_rows_q8(k.float().reshape(-1, 64).numpy()))).view(k.shape)
    assert ko.dtype == torch.float64 and torch.equal(ko, want.double()) and not torch.equal(vo, v)
    k2, _ = cache.update(k[:, :, :1], v[:, :, :1], 0)
    assert k2.shape == (1, 2, 4, 64) and torch.equal(k2[:, :, :3], ko) and torch.equal(k2[:, :, 3], ko[:, :, 0])


# ------------------------------------------------------------------ the server (CPU)
def test_cpu_server_serves_an_int8_kv_tenant_and_reports_a_full_context(model, tmp_path):
    """Nothing new on the server beyond allocating and zeroing the two new state kinds: generate (both
    loops), reset and the overflow report work as on an fp32-KV tenant, and the reply's counters are the
    positions alone (neither the int8 caches nor the scales)."""
    from nos_amd.podserver.client import PodClient, PodServerError
    from nos_amd.podserver.server import PodServer

    progs, w = llama_decode_programs(model, 8, 16, kv="int8")
    prompt = np.random.default_rng(4).integers(0, 512, (1, 8)).astype(np.int32)
    srv = PodServer(tmp_path / "s.sock", device="cpu", lanes=2, memory_gb=40).start()
    try:
        c = PodClient(srv.path, connect_timeout_s=5)
        c.register("llm-kvq8", progs[0], w, memory_limit_gb=1, variants=progs[1:])
        ids, tm = c.generate(prompt, 8, server_loop=True)          # positions 8 .. 15: the cache's last row
        assert tm["state"] == {"pos": [15]}
        assert c.reset()["state"] == {"pos": [0]}
        again, tm2 = c.generate(prompt, 8, server_loop=False)
        assert np.array_equal(again, ids) and tm2["state"] == {"pos": [15]}
        c.infer(ids[:, -1:], outputs=[1])                          # writes row 15: position 16 = full
        with pytest.raises(PodServerError, match="context full"):
            c.infer(ids[:, -1:], outputs=[1])
        c.reset()
        assert np.array_equal(c.generate(prompt, 8)[0], ids)       # and serves a fresh sequence
        c.close()
    finally:
        srv.stop()
