"""Sliding-window attention for decoder tenants on ring K / V caches, on the CPU: the index helpers
the kernels use (through the library's host wrappers), the new entry points' argument checks, the
validator, the eager references against banded attention over the full history, the builder, and
a whole Mistral tenant against ``MistralForCausalLM``.

The rule: the query at position p attends the positions max(0, p - W + 1) .. p.  A ring of C slots
keeps position p in slot p % C; a step of S rows writes its rows and then attends, which is right
for C >= W + S - 1.  After a step ending at pmax slot s holds a(s) = pmax - ((pmax - s) mod C).

The attention oracle is banded attention in fp64 over the full K / V history the test keeps itself
(through ``quantize_kv_rows`` / ``dequantize_kv_rows`` for int8 caches, rounded for bf16), never
the ring reference under test.  The tenant's oracle is the HF model's own forward over the whole
sequence in fp64 (a full recompute: ``kv_q8_roundtrip_cache`` is a ``DynamicCache`` whose layers
are not Mistral's sliding ones, so the int8 tenant is compared against the fp64 recompute with the
round trip applied to K and V by a hook instead)."""
from __future__ import annotations

import copy
import hashlib
import json
import math

import numpy as np
import pytest
import torch

from nos_amd.models.llama_program import (llama_config, llama_decode_programs, llama_model, mistral_config,
                                          mistral_model, mixtral_config, mixtral_model)
from nos_amd.podserver import program as PG
from nos_amd.podserver.program import Builder
from nos_amd.podserver.program.reference import (dequantize_kv_rows, kv_write_ref, quantize_kv_rows,
                                                 sdpa_cache_ref)

INVALID = 1  # hipErrorInvalidValue


@pytest.fixture(scope="module")
def lib():
    from nos_amd.ops import _lib

    return _lib.lib()


# ------------------------------------------------------------------ the rule, transcribed
def held(s, pmax, C):
    return pmax - ((pmax - s) % C)          # Python's % is the non-negative mod


def visible(s, qpos, pmax, C, W):
    a = held(s, pmax, C)
    return a >= 0 and a <= qpos and a > qpos - W


def test_index_helpers_follow_the_rule(lib):
    n = 0
    for C in range(1, 21):
        limit = 3 * C + 1
        for p in range(-3, 3 * C + 3):
            want = -1 if p < 0 or p >= limit else p % C
            assert lib.nos_ring_slot(p, C, limit) == want, (p, C, limit)
        assert lib.nos_ring_slot(C, C, C) == -1 and lib.nos_ring_slot(C - 1, C, C) == C - 1
        for pmax in range(-3, 3 * C + 3):
            pos_of = [lib.nos_ring_position(s, pmax, C) for s in range(C)]
            assert pos_of == [held(s, pmax, C) for s in range(C)], (pmax, C)
            for W in range(1, C + 1):
                for S in range(1, C - W + 2):
                    p0 = pmax - S + 1
                    for qi in range(S):
                        got = [bool(lib.nos_ring_visible(s, p0 + qi, pmax, C, W)) for s in range(C)]
                        assert got == [visible(s, p0 + qi, pmax, C, W) for s in range(C)], (C, W, S, pmax, qi)
                        n += C
    assert n > 100000


def test_split_rows_reach_the_last_slot_a_launch_sees(lib):
    """``ring_oldest`` / ``ring_split_rows`` (a split's live rows) against the per-slot rule, for launches that
    are a whole step or a part of one, splits of 1 .. C slots."""
    for C in (1, 2, 5, 8, 13):
        for W in range(1, C + 1):
            for S in range(1, C - W + 2):
                for p0 in range(0, 3 * C):
                    pmax = p0 + S - 1
                    for q0, sq in {(0, S), (0, 1), (S - 1, 1), (S // 2, S - S // 2)}:
                        lo = lib.nos_ring_oldest(p0 + q0, pmax, C, W)
                        hi = p0 + q0 + sq - 1
                        seen = [any(visible(s, p0 + q0 + i, pmax, C, W) for i in range(sq)) for s in range(C)]
                        assert seen == [lo <= held(s, pmax, C) <= hi for s in range(C)]
                        for n in {1, 3, C}:
                            for k0 in range(0, C, n):
                                m = min(n, C - k0)
                                want = max([j + 1 for j in range(m) if seen[k0 + j]], default=0)
                                assert lib.nos_ring_split_rows(k0, m, lo, hi, C) == want, (C, W, S, p0, q0, sq, k0, m)


# ------------------------------------------------------------------ entry points: argument checks
def _p(i: int) -> int:
    return 0x100000 * (i + 1)    # a dummy aligned device pointer (nothing is dereferenced)


def _write_args(**kw):
    a = dict(x=_p(0), xbf=0, ldx=128, bsx=3 * 128, cache=_p(1), cbf=0, pos=_p(2), cos=None, sin=None, R=0, B=2, S=3,
             H=2, D=64, C=12, x2=None, ldx2=0, bsx2=0, cache2=None, window=8, limit=40, stream=None)
    a.update(kw)
    return list(a.values())


def _write_q8_args(**kw):
    a = dict(x=_p(0), ldx=128, bsx=3 * 128, cache=_p(1), scales=_p(3), deq=None, pos=_p(2), cos=None, sin=None, R=0,
             B=2, S=3, H=2, D=64, C=12, x2=None, ldx2=0, bsx2=0, cache2=None, scales2=None, deq2=None, window=8,
             limit=40, stream=None)
    a.update(kw)
    return list(a.values())


def _attn_args(lib, q8=False, **kw):
    B, H, Hkv, Sq, C, D = 2, 4, 2, 3, 12, 64
    a = dict(q=_p(0), qbf=0, ldq=H * D, bsq=Sq * H * D, kc=_p(1), vc=_p(2), cbf=0, ks=_p(5), vs=_p(6), pos=_p(3),
             cos=None, sin=None, R=0, out=_p(4), obf=0, B=B, H=H, Hkv=Hkv, Sq=Sq, C=C, D=D, scale=0.125, ws=_p(7),
             ws_bytes=1 << 30, kn=None, vn=None, nbf=0, ldk=0, bsk=0, ldv=0, bsv=0, nfresh=0, sync=None, sync_n=0,
             partials=0, window=8, limit=40, stream=None)
    a.update(kw)
    drop = ("qbf", "cbf", "obf", "nbf") if q8 else ("ks", "vs")
    return [v for k, v in a.items() if k not in drop]


RING_DEFECTS = [("window = 0", dict(window=0)), ("C below window + S - 1", dict(window=11)),
                ("C above limit", dict(limit=11)), ("limit = 0", dict(limit=0)),
                ("limit above the rotary tables", dict(cos=_p(8), sin=_p(9), R=39))]


@pytest.mark.parametrize("what, kw", RING_DEFECTS)
def test_ring_entry_points_refuse_bad_arguments(lib, what, kw):
    assert lib.nos_kv_write_ring(*_write_args(**kw)) == INVALID, what
    assert lib.nos_kv_write_ring_q8(*_write_q8_args(**kw)) == INVALID, what
    assert lib.nos_attn_decode_ring(*_attn_args(lib, **kw)) == INVALID, what
    assert lib.nos_attn_decode_ring_q8(*_attn_args(lib, q8=True, **kw)) == INVALID, what


def test_ring_entry_points_keep_the_plain_checks(lib):
    assert lib.nos_kv_write_ring(*_write_args(x=None)) == INVALID
    assert lib.nos_kv_write_ring(*_write_args(S=13)) == INVALID           # more rows than slots
    assert lib.nos_kv_write_ring_q8(*_write_q8_args(D=96)) == INVALID
    assert lib.nos_kv_write_ring_q8(*_write_q8_args(scales=None)) == INVALID
    assert lib.nos_attn_decode_ring(*_attn_args(lib, cbf=2)) == INVALID   # int8 caches have their own entry point
    assert lib.nos_attn_decode_ring(*_attn_args(lib, ws_bytes=16)) == INVALID
    assert lib.nos_attn_decode_ring_q8(*_attn_args(lib, q8=True, ks=None)) == INVALID
    # C = limit < window + S - 1 is a whole cache, not a defect: min(limit, window + S - 1) slots suffice --
    # the only thing wrong with these calls is the null q
    assert lib.nos_attn_decode_ring(*_attn_args(lib, q=None, window=100, limit=12)) == INVALID


# ------------------------------------------------------------------ validator
VB, VC, VHKV, VD, VH, VS = 2, 12, 2, 64, 4, 3


def _prog(kdt="fp32", S=VS, C=VC, k_attrs=None, v_attrs=None, a_attrs=None, sc_shape=None):
    ring = dict(window=8, limit=40)
    k_attrs, v_attrs, a_attrs = (ring if t is None else t for t in (k_attrs, v_attrs, a_attrs))
    b = Builder("ring")
    x = b.input("x", [VB, S, (VH + 2 * VHKV) * VD], "fp32")
    b.state("pos", [VB], "i32")
    kc, vc = b.state("kc", [VB, C, VHKV, VD], kdt), b.state("vc", [VB, C, VHKV, VD], kdt)
    sc = []
    if kdt == "i8":
        b.state("ks", list(sc_shape or (VB, C, VHKV)), "fp32")
        b.state("vs", [VB, C, VHKV], "fp32")
        sc = [["ks"], ["vs"]]
    q = b.op("reshape", b.op("slice", x, dim=-1, start=0, end=VH * VD), shape=[VB, S, VH, VD])
    k = b.op("reshape", b.op("slice", x, dim=-1, start=VH * VD, end=(VH + VHKV) * VD), shape=[VB, S, VHKV, VD])
    v = b.op("reshape", b.op("slice", x, dim=-1, start=(VH + VHKV) * VD, end=(VH + 2 * VHKV) * VD),
             shape=[VB, S, VHKV, VD])
    kc1 = b.op("kv_write", kc, k, "pos", *(sc[0] if sc else []), **k_attrs)
    vc1 = b.op("kv_write", vc, v, "pos", *(sc[1] if sc else []), **v_attrs)
    o = b.op("sdpa_cache", q, kc1, vc1, "pos", *(sc[0] + sc[1] if sc else []), **a_attrs)
    return b.build([o])


def test_validator_takes_ring_caches():
    for kdt in ("fp32", "i8"):
        p = PG.parse(*_prog(kdt))
        assert [n.attrs for n in p.nodes if n.op in ("kv_write", "sdpa_cache")] == [dict(window=8, limit=40)] * 3
        assert p.state["kc"].shape == (VB, VC, VHKV, VD)
    PG.parse(*_prog(C=10, S=3))                                                  # C = window + S - 1 exactly
    PG.parse(*_prog(C=12, k_attrs=dict(window=100, limit=12), v_attrs=dict(window=100, limit=12),
                    a_attrs=dict(window=100, limit=12)))                          # C = limit: the whole context
    PG.parse(*_prog(k_attrs={}, v_attrs={}, a_attrs={}))                         # and without them nothing changes


@pytest.mark.parametrize("kw, msg", [
    (dict(k_attrs=dict(window=8)), "window and limit are given together"),
    (dict(a_attrs=dict(limit=40)), "window and limit are given together"),
    (dict(C=9), r"needs min\(limit, window \+ S - 1\) = 10 slots"),
    (dict(k_attrs=dict(window=8, limit=11), v_attrs=dict(window=8, limit=11), a_attrs=dict(window=8, limit=11)),
     "longer than its limit 11"),
    (dict(k_attrs=dict(window=0, limit=40)), "window must be an int >= 1"),
    (dict(k_attrs=dict(window=8, limit=True)), "limit must be an int >= 1"),
    (dict(a_attrs=dict(window=7, limit=40)), "is a ring of window 8 and limit 40 in an earlier node and a ring of "
                                             "window 7 and limit 40 here"),
    (dict(a_attrs={}), "in an earlier node and a plain cache here"),
    (dict(k_attrs={}), None),      # K plain and V a ring: the attention disagrees with one of them
    (dict(kdt="i8", sc_shape=(VB, 40, VHKV)), r"scales of an i8 cache must be an fp32 \[2, 12, 2\] state"),
])
def test_validator_refusals(kw, msg):
    with pytest.raises(PG.ProgramError, match=msg):
        PG.parse(*_prog(**kw))


# ------------------------------------------------------------------ the references against banded attention
def banded64(q, kh, vh, p0, W, scale):
    """q [Sq, H, D] at positions p0 + i over the full history kh / vh [T, Hkv, D] (T > p0 + Sq - 1), fp64."""
    Sq, H, D = q.shape
    G = H // kh.shape[1]
    out = torch.zeros(Sq, H, D, dtype=torch.float64)
    for i in range(Sq):
        p = p0 + i
        lo = max(0, p - W + 1)
        k = kh[lo:p + 1].double().repeat_interleave(G, dim=1)
        v = vh[lo:p + 1].double().repeat_interleave(G, dim=1)
        s = torch.einsum("hd,khd->hk", q[i].double(), k) * scale
        out[i] = torch.einsum("hk,khd->hd", torch.softmax(s, -1), v)
    return out


def _as_cache(x, kind):
    """The history as a cache of ``kind`` holds it."""
    if kind == "int8":
        return dequantize_kv_rows(*quantize_kv_rows(x))
    return x.to(torch.bfloat16).float() if kind == "bf16" else x


MIXED = [1, 1, 3, 4, 2, 2] * 6 + [2]           # chunks of 1 .. 4 tokens over 80 positions
assert sum(MIXED) == 80
CHUNKS = {"prefill5-steps": ([5] + [1] * 30, 8), "mixed": (MIXED, 6), "w1": ([3, 1, 2, 1, 1, 3], 1),
          "wide-window": ([4] * 12, 193)}


@pytest.mark.parametrize("kind", ["fp64", "fp32", "bf16", "int8"])
@pytest.mark.parametrize("name", list(CHUNKS))
def test_ring_references_are_banded_attention_over_the_history(name, kind):
    chunks, W = CHUNKS[name]
    B, Hkv, H, D = 2, 2, 4, 16
    T, smax = sum(chunks), max(chunks)
    limit = T + 7
    C = min(limit, W + smax - 1)
    g = torch.Generator().manual_seed(len(name) + W)
    dt = torch.float64 if kind == "fp64" else torch.float32
    kh, vh = torch.randn(B, T, Hkv, D, generator=g, dtype=dt), torch.randn(B, T, Hkv, D, generator=g, dtype=dt)
    qh = torch.randn(B, T, H, D, generator=g, dtype=dt)
    cdt = {"fp64": torch.float64, "fp32": torch.float32, "bf16": torch.bfloat16, "int8": torch.int8}[kind]
    kc, vc = (torch.full((B, C, Hkv, D), 99 if kind == "int8" else float("nan")).to(cdt) for _ in range(2))
    ks, vs = (torch.full((B, C, Hkv), float("nan")) for _ in range(2)) if kind == "int8" else (None, None)
    kw = dict(window=W, limit=limit)
    t, worst, wraps = 0, 0.0, 0
    scale = 1 / math.sqrt(D)
    for S in chunks:
        pos = torch.tensor([t, t], dtype=torch.int32)
        assert kv_write_ref(kc, kh[:, t:t + S], pos, ks, **kw) is kc
        kv_write_ref(vc, vh[:, t:t + S], pos, vs, **kw)
        got = sdpa_cache_ref(qh[:, t:t + S], kc, vc, pos, scale, ks, vs, **kw)
        assert got.dtype == dt and got.shape == (B, S, H, D)
        for b in range(B):
            want = banded64(qh[b, t:t + S], _as_cache(kh[b], kind), _as_cache(vh[b], kind), t, W, scale)
            worst = max(worst, float((got[b].double() - want).abs().max()))
        wraps += t // C != (t + S) // C
        t += S
    assert wraps >= (0 if name == "wide-window" else 2), "the ring must wrap, inside a step or between two"
    print(f"{name} {kind}: e = {worst:.3g}")
    assert worst <= (1e-13 if kind == "fp64" else 2e-6), worst


def test_ring_references_drop_rows_outside_the_limit_and_zero_a_bad_counter():
    g = torch.Generator().manual_seed(3)
    C, W, limit = 6, 4, 9
    x = torch.randn(3, 3, 1, 8, generator=g)
    cache = torch.full((3, C, 1, 8), 7.0)
    kv_write_ref(cache, x, torch.tensor([-1, 7, 9], dtype=torch.int32), window=W, limit=limit)
    assert torch.equal(cache[0, 0], x[0, 1]) and torch.equal(cache[0, 1], x[0, 2]) and bool((cache[0, 2:] == 7).all())
    assert torch.equal(cache[1, 1], x[1, 0]) and torch.equal(cache[1, 2], x[1, 1])       # 7 -> slot 1, 8 -> slot 2, 9 dropped
    assert bool((cache[1, [0, 3, 4, 5]] == 7).all()) and bool((cache[2] == 7).all())
    q = torch.randn(3, 1, 2, 8, generator=g)
    out = sdpa_cache_ref(q, cache, cache, torch.tensor([-1, 3, 9], dtype=torch.int32), window=W, limit=limit)
    assert not out[0].any() and not out[2].any() and bool(out[1].any())
    for bad in (dict(window=W), dict(limit=limit), dict(window=0, limit=limit), dict(window=W, limit=5),
                dict(window=5, limit=limit)):
        with pytest.raises(ValueError):
            kv_write_ref(cache, x, torch.zeros(3, dtype=torch.int32), **bad)


# ------------------------------------------------------------------ builder
MAX_LEN = 48
SEED = 0


@pytest.fixture(scope="module")
def model():
    return mistral_model(mistral_config(), SEED)


# sha256 of json.dumps(programs, sort_keys=True) as the builder produced them before it knew a window
# (tests/test_moe.py pins the same Llama sets); "mistral": a MistralForCausalLM with sliding_window=None
PINS = {"plain": (dict(), "e6f4d1d223b688cf989d9a7d0fa543da65342f30ffb7e58cb177d6e7ae69d17e"),
        "kvq8-speculate": (dict(kv="int8", speculate=4), "0df8bcdc0796b2651ea5dbfdd9bf6f23c7c0878c6e499b4bcc273dab0401e896"),
        "bf16": (dict(dtype="bf16"), "b224160db818d5accef296b899b798861472d1c7b2c918a8e22eee83e86e202c")}
MISTRAL_PIN = PINS["plain"][0 + 1]     # the same shapes and names as the tiny Llama: the same serialisation


def _sha(progs):
    return hashlib.sha256(json.dumps(progs, sort_keys=True).encode()).hexdigest()


def test_programs_without_an_effective_window_are_unchanged():
    m = llama_model(llama_config(False), 0)
    for name, (kw, pin) in PINS.items():
        assert _sha(llama_decode_programs(m, 16, 64, **kw)[0]) == pin, name
        assert _sha(llama_decode_programs(m, 16, 64, window=64, **kw)[0]) == pin, name      # window >= max_len
        assert _sha(llama_decode_programs(m, 16, 64, window=1000, **kw)[0]) == pin, name
        assert _sha(llama_decode_programs(m, 16, 64, window=63, **kw)[0]) != pin, name
    ms = mistral_model(mistral_config(sliding_window=None), 0)
    progs, w = llama_decode_programs(ms, 16, 64)
    assert _sha(progs) == MISTRAL_PIN
    mw = mistral_model(mistral_config(sliding_window=64), 0)      # the config's window, not below max_len
    assert llama_decode_programs(mw, 16, 64) == (progs, w)
    assert llama_decode_programs(ms, 16, 64, window=64) == (progs, w)


def test_builder_sizes_one_ring_for_every_variant(model):
    for kw, C in [(dict(), 8 + 5 - 1), (dict(extend=(4, 9)), 8 + 9 - 1), (dict(speculate=4), 12),
                  (dict(prompt_len=2), 9), (dict(prompt_len=44), MAX_LEN), (dict(window=3), 7),
                  (dict(window=1, prompt_len=2), 2), (dict(kv="int8", batch=2), 12), (dict(dtype="bf16"), 12)]:
        kw = dict(kw)
        progs, w = llama_decode_programs(model, kw.pop("prompt_len", 5), MAX_LEN, **kw)
        W = kw.get("window", 8)
        for p in PG.parse_variants(progs, w):
            B = kw.get("batch", 1)
            assert p.state["kc0"].shape == (B, C, 1, 128) and p.state["vc1"].shape == (B, C, 1, 128), (kw, C)
            if kw.get("kv") == "int8":
                assert p.state["ks0"].shape == (B, C, 1)
            if kw.get("speculate"):
                assert p.state["hist"].shape == (B, MAX_LEN)
            assert p.params["rope.cos"].shape == (MAX_LEN, 128)
            ring = [n.attrs for n in p.nodes if n.op in ("kv_write", "sdpa_cache")]
            assert len(ring) == 6 and all(a.get("window") == W and a.get("limit") == MAX_LEN for a in ring)
    # an explicit window overrides the config's; None on a Llama means none
    assert llama_decode_programs(model, 5, MAX_LEN, window=8) == llama_decode_programs(model, 5, MAX_LEN)
    lm = llama_model(llama_config(False), 0)
    assert all("window" not in n.get("attrs", {}) for p in llama_decode_programs(lm, 5, MAX_LEN)[0] for n in p["nodes"])
    assert llama_decode_programs(lm, 5, MAX_LEN, window=8)[0][0]["state"][1]["shape"] == [1, 12, 1, 128]


def test_builder_refusals(model):
    for bad in (0, -3, 2.5, True, "8"):
        with pytest.raises(ValueError, match="window must be an int >= 1"):
            llama_decode_programs(model, 5, MAX_LEN, window=bad)
    mx = mixtral_model(mixtral_config(num_hidden_layers=1), 0)
    with pytest.raises(ValueError, match="a Mixtral tenant takes no window"):
        llama_decode_programs(mx, 5, MAX_LEN, window=8)
    with pytest.raises(ValueError, match="a Mixtral tenant takes no window"):
        llama_decode_programs(mx, 5, MAX_LEN, window=MAX_LEN)
    mxw = mixtral_model(mixtral_config(num_hidden_layers=1, sliding_window=8), 0)
    with pytest.raises(ValueError, match="sliding_window = 8 is set and smaller than max_len = 48"):
        llama_decode_programs(mxw, 5, MAX_LEN)


def test_estimate_and_state_bytes_follow_the_ring(model):
    full = copy.deepcopy(model)
    full.config.sliding_window = None
    pf = PG.parse_variants(*llama_decode_programs(full, 5, MAX_LEN))
    pw = PG.parse_variants(*llama_decode_programs(model, 5, MAX_LEN))
    C, layers = 12, model.config.num_hidden_layers
    row = 1 * 128 * 4                                  # one (position, KV head) row of one fp32 cache
    saved = 2 * layers * (MAX_LEN - C) * row
    for a, b in zip(pf, pw):
        assert b.state_bytes == a.state_bytes - saved
    assert pw[1].bytes_estimate == pf[1].bytes_estimate - saved         # a step: the states and nothing else
    cache_bytes = lambda ps: sum(v.nbytes for k, v in ps[1].state.items() if k[:2] in ("kc", "vc"))  # noqa: E731
    assert cache_bytes(pw) * MAX_LEN == cache_bytes(pf) * C
    p8 = PG.parse_variants(*llama_decode_programs(model, 5, MAX_LEN, kv="int8"))
    assert sum(v.nbytes for k, v in p8[1].state.items() if k[:2] in ("kc", "vc", "ks", "vs")) == 2 * layers * C * (128 + 4)


# ------------------------------------------------------------------ a Mistral tenant on the CPU
def _ids(n, batch=1, seed=SEED):
    return torch.randint(0, 512, (batch, n), generator=torch.Generator().manual_seed(seed + 11), dtype=torch.int32)


def _compiled(model, prompt_len, **kw):
    progs, w = llama_decode_programs(model, prompt_len, MAX_LEN, **kw)
    ps = PG.parse_variants(progs, w)
    params, state = ps[0].tensors("cpu"), ps[0].state_tensors("cpu")
    return [p.compile("cpu", params=params, state=state) for p in ps], state, ps


def _hf_logits(m, ids, rows):
    """The HF model's logits at ``rows`` of one forward over the whole sequence."""
    with torch.no_grad():
        return m(ids.long()).logits[:, rows]


def _bar(got, model, ids, rows, what, ref_model=None):
    """The tenant tests' logit bar: e <= max(4 e32, 1e-5) relative to the largest logit, against the HF model in
    fp64; returns (fp64 logits, the worst fp32-side error per row) for the tie check."""
    base = ref_model or model
    r64 = _hf_logits(copy.deepcopy(base).double(), ids, rows)
    r32 = _hf_logits(base, ids, rows)
    scale = float(r64.abs().max())
    e = float((got.double() - r64).abs().max()) / scale
    e32 = float((r32.double() - r64).abs().max()) / scale
    print(f"{what}: e = {e:.3g}, e32 = {e32:.3g}")
    assert got.shape == r64.shape and e <= max(4 * e32, 1e-5), (what, e, e32)
    return r64, (got.double() - r64).abs().amax(dim=-1)


def _no_ties(r64, err, what):
    """No compared step's top-2 logit gap (fp64) is below twice the fp32 error observed there."""
    top = r64.topk(2, dim=-1).values
    gap = top[..., 0] - top[..., 1]
    assert bool((gap > 2 * err).all()), (what, float(gap.min()), float(err.max()))


def _feed(progs_by_len, ids, plan):
    """Run ``plan`` (chunk lengths) of teacher-forced ids through the variants; the logits of each chunk's last row."""
    out, t = [], 0
    with torch.no_grad():
        for n in plan:
            out.append(progs_by_len[n](ids[:, t:t + n])[0])
            t += n
    return torch.cat(out, 1)


@pytest.mark.parametrize("plan", [[5] + [1] * 30, [20] + [1] * 6, [5, 4] + [1] * 8], ids=["wraps", "S>W", "extend"])
def test_mistral_tenant_is_the_hf_model(model, plan):
    batch = 2 if plan[0] == 5 and plan[1] == 1 else 1
    ids = _ids(sum(plan), batch)
    extend = (4,) if 4 in plan else ()
    comp, state, ps = _compiled(model, plan[0], batch=batch, extend=extend)
    by_len = {c.program.inputs[0].shape[1]: c for c in comp}
    C = min(MAX_LEN, 8 + max(plan[0], *extend, 1) - 1)
    assert state["kc0"].shape == (batch, C, 1, 128) and comp[1].stats["ring_caches"] == 4
    got = _feed(by_len, ids, plan)
    assert state["pos"].tolist() == [sum(plan)] * batch
    rows = (np.cumsum(plan) - 1).tolist()
    r64, err = _bar(got, model, ids, rows, f"mistral {plan[:2]}")
    _no_ties(r64, err, plan)
    assert torch.equal(got.argmax(-1), r64.argmax(-1))
    # the prefill of a prompt within the window attends with the flash kernel's op, a longer one keeps the ring
    kinds = [s.kind for s in comp[0].steps]
    assert ("sdpa" in kinds, "sdpa_cache" in kinds) == ((True, False) if plan[0] <= 8 else (False, True))
    # a full-attention twin differs from the second position past the window on
    twin = copy.deepcopy(model)
    twin.config.sliding_window = None
    tcomp, _, _ = _compiled(twin, plan[0], batch=batch, extend=extend)
    tgot = _feed({c.program.inputs[0].shape[1]: c for c in tcomp}, ids, plan)
    far = [i for i, r in enumerate(rows) if r >= 9]
    assert float((tgot[:, far] - got[:, far]).abs().max()) > 1e-3
    # the eager, unfused reference computes the same from its own state
    rstate = {k: t.clone().zero_() for k, t in state.items()}
    t0, ref = 0, []
    for n in plan[:8]:
        ref.append(ps[[p.inputs[0].shape[1] for p in ps].index(n)].reference(ids[:, t0:t0 + n], state=rstate)[0])
        t0 += n
    torch.testing.assert_close(got[:, :len(ref)], torch.cat(ref, 1), rtol=1e-5, atol=1e-5)


def _generate_hf(model, prompt, n, **kw):
    with torch.no_grad():
        out = model.generate(torch.from_numpy(prompt).long(), max_new_tokens=n, do_sample=False, pad_token_id=0, **kw)
    return out[:, prompt.shape[1]:].numpy()


def _gen_no_ties(model, prompt, toks):
    """Teacher-forced over prompt + generated tokens: the fp64 logits of every generating row have no tie at the
    fp32 model's own error."""
    ids = torch.from_numpy(np.concatenate([prompt, toks], 1)).int()
    rows = list(range(prompt.shape[1] - 1, ids.shape[1] - 1))
    r64 = _hf_logits(copy.deepcopy(model).double(), ids, rows)
    r32 = _hf_logits(model, ids, rows)
    _no_ties(r64, (r32.double() - r64).abs().amax(-1), "generate")
    assert np.array_equal(r64.argmax(-1).numpy(), toks)


def _serve(tmp_path, progs, w, fn, name="swa"):
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    srv = PodServer(tmp_path / f"{name}.sock", device="cpu", lanes=2, memory_gb=40).start()
    try:
        c = PodClient(srv.path, connect_timeout_s=5)
        c.register(name, progs[0], w, memory_limit_gb=1, variants=progs[1:])
        out = fn(c)
        c.close()
        return out
    finally:
        srv.stop()


def test_cpu_server_generates_transformers_tokens(model, tmp_path):
    prompt = np.random.default_rng(4).integers(0, 512, (2, 5)).astype(np.int32)
    want = _generate_hf(model, prompt, 30)
    _gen_no_ties(model, prompt, want)
    progs, w = llama_decode_programs(model, 5, MAX_LEN, batch=2)

    def run(c):
        ids, tm = c.generate(prompt, 30, server_loop=True)
        assert tm["state"] == {"pos": [34, 34]}
        c.reset()
        again, _ = c.generate(prompt, 30, server_loop=False)
        return ids, again

    ids, again = _serve(tmp_path, progs, w, run)
    assert np.array_equal(ids, want) and np.array_equal(again, want)


def test_cpu_server_takes_a_prompt_longer_than_the_window_and_a_prompt_in_chunks(model, tmp_path):
    """A 20-token prompt (S > W: the prefill stays on the ring attention), and a 9-token prompt fed as prefill 5 +
    extend 4: transformers' tokens."""
    rng = np.random.default_rng(8)
    long_p, short_p = (rng.integers(0, 512, (1, n)).astype(np.int32) for n in (20, 9))
    want_long, want_short = _generate_hf(model, long_p, 12), _generate_hf(model, short_p, 20)
    _gen_no_ties(model, long_p, want_long)
    _gen_no_ties(model, short_p, want_short)
    ids = _serve(tmp_path, *llama_decode_programs(model, 20, MAX_LEN), lambda c: c.generate(long_p, 12)[0], "long")
    assert np.array_equal(ids, want_long)

    def chunks(c):
        c.infer(short_p[:, :5], outputs=[1])
        return c.generate(short_p[:, 5:], 20)[0]       # the extend variant takes the prompt's rest, then the loop

    ids = _serve(tmp_path, *llama_decode_programs(model, 5, MAX_LEN, extend=(4,)), chunks, "chunks")
    assert np.array_equal(ids, want_short)


def test_cpu_server_reports_a_full_context_at_max_len_not_at_the_ring(model, tmp_path):
    from nos_amd.podserver.client import PodServerError

    progs, w = llama_decode_programs(model, 5, 20)           # C = 12 slots, 20 positions
    prompt = np.random.default_rng(4).integers(0, 512, (1, 5)).astype(np.int32)

    def run(c):
        ids, tm = c.generate(prompt, 15, server_loop=True)    # positions 5 .. 19 hold the 14 fed-back ids
        assert tm["state"] == {"pos": [19]}
        c.infer(ids[:, -1:], outputs=[1])                     # writes position 19: 20 = full
        with pytest.raises(PodServerError, match="context full"):
            c.infer(ids[:, -1:], outputs=[1])
        return ids

    ids = _serve(tmp_path, progs, w, run)
    assert np.array_equal(ids, _generate_hf(model, prompt, 15))


def test_speculating_windowed_tenant_emits_the_plain_windowed_tenants_tokens(model, tmp_path):
    rng = np.random.default_rng(6)
    prompt = np.tile(rng.integers(0, 512, (1, 6)), (1, 2)).astype(np.int32)[:, :11]   # a repeat: drafts get accepted
    want = _generate_hf(model, prompt, 24)
    _gen_no_ties(model, prompt, want)
    plain = _serve(tmp_path, *llama_decode_programs(model, 11, MAX_LEN), lambda c: c.generate(prompt, 24)[0], "plain")
    progs, w = llama_decode_programs(model, 11, MAX_LEN, speculate=4)
    assert PG.parse_variants(progs, w)[0].state["kc0"].shape == (1, 8 + 11 - 1, 1, 128)

    def run(c):
        ids, tm = c.generate(prompt, 24, speculate=True)
        return ids, tm

    ids, tm = _serve(tmp_path, progs, w, run, "spec")
    assert np.array_equal(plain, want) and np.array_equal(ids, want)
    print("speculation:", {k: v for k, v in tm.items() if "step" in k or "acc" in k})


def test_stopping_windowed_tenant_emits_transformers_tokens(model, tmp_path):
    prompt = np.random.default_rng(4).integers(0, 512, (2, 5)).astype(np.int32)
    free = _generate_hf(model, prompt, 30)
    stop = [int(free[0, 12]), int(free[1, 20])]               # ids the rows emit past the window
    want = _generate_hf(model, prompt, 30, eos_token_id=stop, repetition_penalty=1.0)
    progs, w = llama_decode_programs(model, 5, MAX_LEN, batch=2, stopping=True)
    ids = _serve(tmp_path, progs, w, lambda c: c.generate(prompt, 30, eos_token_id=stop, pad_token_id=0)[0])
    assert want.shape[1] < 30 and np.array_equal(ids, want), (ids.shape, want.shape)
    _gen_no_ties(model, prompt[:1], free[:1, :13])
    _gen_no_ties(model, prompt[1:], free[1:, :21])


def _q8_roundtrip_hooks(m):
    """K (after its rotation) and V of every layer through the int8 cache's round trip, per token and KV head: the
    model an int8-KV tenant computes, as a full recompute (eager attention receives K and V as keyword arguments)."""
    import transformers.models.mistral.modeling_mistral as mm

    orig = mm.eager_attention_forward

    def wrapped(module, query, key, value, *a, **kw):
        rt = lambda x: dequantize_kv_rows(*quantize_kv_rows(x)).to(x.dtype)  # noqa: E731
        return orig(module, query, rt(key), rt(value), *a, **kw)

    return mm, orig, wrapped


def test_int8_kv_windowed_tenant_is_the_recompute_with_the_round_trip(model, monkeypatch):
    plan = [5] + [1] * 20
    ids = _ids(sum(plan))
    comp, state, _ = _compiled(model, 5, kv="int8")
    assert state["kc0"].dtype == torch.int8 and state["ks0"].shape == (1, 12, 1)
    assert comp[1].stats["ring_caches"] == 4 and comp[1].stats["kv_q8_caches"] == 4
    got = _feed({c.program.inputs[0].shape[1]: c for c in comp}, ids, plan)
    mm, orig, wrapped = _q8_roundtrip_hooks(model)
    monkeypatch.setattr(mm, "eager_attention_forward", wrapped)
    model.config._attn_implementation = "eager"
    # the HF modules look the attention function up by name at call time
    if hasattr(mm, "ALL_ATTENTION_FUNCTIONS"):
        pass
    rows = (np.cumsum(plan) - 1).tolist()
    r64, err = _bar(got, model, ids, rows, "mistral kv int8")
    monkeypatch.setattr(mm, "eager_attention_forward", orig)
    plain64 = _hf_logits(copy.deepcopy(model).double(), ids, rows)
    assert float((plain64 - r64).abs().max()) > 1e-4, "the round trip must have been applied"
