"""Int8 K / V caches on the GPU (csrc/hip/decode.hip: ``kv_write_q8_kernel`` and the
``CBF == 2`` instantiations of ``attn_decode_kernel``), and int8-KV decoder tenants
compiled for the GPU and served with HIP graphs.

A cache row is D int8 values and one fp32 scale, ``quantize_rows_q8``'s rule on the
row in fp32; the cache holds ``float(q) * scale`` and everything that attends it
computes exact fp32 arithmetic on those values -- so the attention is held to the
fp32 cache's bar, max |got - ref64| <= max(4 e32, 2e-6) against fp64 on the
dequantized caches, and every statement about stored bytes is bit-exact.

Inputs are drawn on the CPU from seeded generators; references run on the CPU."""
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
from nos_amd.podserver.program import dequantize_rows_q8, quantize_rows_q8  # noqa: E402
from nos_amd.podserver.program.reference import rotary_at_ref, sdpa_cache_ref  # noqa: E402

F32, I8 = torch.float32, torch.int8
B, L, HKV = 2, 300, 2          # three 128-key splits, the last one partial


@pytest.fixture(autouse=True)
def _h3():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).cuda()


def _pos(*v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _tables(n, d):
    inv = 1.0 / 10000 ** (torch.arange(0, d, 2, dtype=torch.float64) / d)
    f = torch.outer(torch.arange(n, dtype=torch.float64), inv)
    e = torch.cat([f, f], 1)
    return e.cos().float().cuda(), e.sin().float().cuda()


def _rot64(x, tabs, pos):
    """``rotary_at_ref`` in fp64 (on the fp32 tables' values)."""
    if tabs is None:
        return x.double().cpu()
    b, S, H, D = x.shape
    c, s = tabs[0].double().cpu(), tabs[1].double().cpu()
    idx = (pos.cpu().long().view(b, 1) + torch.arange(S).view(1, S)).clamp(0, c.shape[0] - 1)
    xd = x.double().cpu()
    rot = torch.cat([-xd[..., D // 2:], xd[..., :D // 2]], dim=-1)
    return xd * c[idx][:, :, None, :] + rot * s[idx][:, :, None, :]


def _quant(x):
    """``quantize_rows_q8`` of the rows x [..., D] (CPU): (int8 [..., D], fp32 [...])."""
    q, s = quantize_rows_q8(x.detach().cpu().float().reshape(-1, x.shape[-1]).numpy())
    return torch.from_numpy(q).view(x.shape), torch.from_numpy(s).view(x.shape[:-1])


def _deq(q, s):
    out = dequantize_rows_q8(q.cpu().reshape(-1, q.shape[-1]).numpy(), s.cpu().reshape(-1).numpy())
    return torch.from_numpy(out).view(q.shape)


def _caches(g, b, D, hkv=HKV):
    """Given i8 caches: random int8 values and positive scales spanning 2^-6 .. 2^6 over the rows."""
    kc = torch.randint(-127, 128, (b, L, hkv, D), generator=g, dtype=I8).cuda()
    vc = torch.randint(-127, 128, (b, L, hkv, D), generator=g, dtype=I8).cuda()
    ks = torch.exp2(12 * torch.rand(b, L, hkv, generator=g) - 6).cuda()
    vs = torch.exp2(12 * torch.rand(b, L, hkv, generator=g) - 6).cuda()
    return kc, vc, ks, vs


# ------------------------------------------------------------------ 1, 2. the quantizing write
@pytest.mark.parametrize("D", [64, 128])
def test_kv_write_stores_the_rows_quantized_bit_for_bit(D):
    """No rotation: bytes, scales and the ``deq`` output are ``quantize_rows_q8``'s /
    ``dequantize_rows_q8``'s, bit for bit; x a strided slice of a fused projection; the
    last sequence overflows the cache (its rows past L are dropped); K and V in one launch."""
    b, S = 3, 5
    g = _gen(D)
    proj = _randn(g, b, S, 3 * HKV * D) * torch.logspace(-2, 2, b * S).view(b, S, 1).cuda()
    x = proj[..., HKV * D:2 * HKV * D].view(b, S, HKV, D)
    x2 = _randn(g, b, S, HKV, D)
    x2[1, 2, 1] = 0                                    # an all-zero row: scale 1
    assert not x.is_contiguous()
    pos = _pos(0, 17, L - 2)
    cache, cache2 = (torch.full((b, L, HKV, D), 77, dtype=I8, device="cuda") for _ in range(2))
    scales, scales2 = (torch.full((b, L, HKV), -5.0, device="cuda") for _ in range(2))
    got, dq, dq2 = T.kv_write(cache, x, pos, second=(cache2, x2, scales2), scales=scales, deq=True)
    torch.cuda.synchronize()
    assert got is cache
    for c, s, d, xx in ((cache, scales, dq, x), (cache2, scales2, dq2, x2)):
        q, sc = _quant(xx)
        c, s, d = c.cpu(), s.cpu(), d.cpu()
        untouched = torch.ones(b, L, dtype=torch.bool)
        for i, p in enumerate(pos.tolist()):
            n = min(S, L - p)
            assert torch.equal(c[i, p:p + n], q[i, :n]) and torch.equal(s[i, p:p + n], sc[i, :n]), (i, p)
            assert torch.equal(d[i, :n], _deq(q, sc)[i, :n])
            untouched[i, p:p + n] = False
        assert bool((c[untouched] == 77).all()) and bool((s[untouched] == -5.0).all())
    assert float(scales2[1, 17 + 2, 1]) == 1.0 and not bool(cache2[1, 17 + 2, 1].any())
    # a single write is the pair's first half
    c1, s1 = torch.full_like(cache, 77), torch.full_like(scales, -5.0)
    assert T.kv_write(c1, x, pos, scales=s1) is c1 and torch.equal(c1, cache) and torch.equal(s1, scales)


@pytest.mark.parametrize("D", [64, 128])
def test_kv_write_rotates_then_quantizes(D):
    """With rotary, against the rows rotated in fp64 on the fp32 tables: the scale is the
    rotated row's maximum / 127 to fp32 round-off, and every element lies within half a
    quantization step (plus the fp32 rotation's error) of the fp64 value -- a property of
    any correct rounding; no share of the elements is exempt."""
    b, S = 3, 5
    g = _gen(D + 1)
    x = _randn(g, b, S, HKV, D)
    pos = _pos(0, 17, L - 2 - S)
    tabs = _tables(L, D)
    cache = torch.zeros(b, L, HKV, D, dtype=I8, device="cuda")
    scales = torch.zeros(b, L, HKV, device="cuda")
    _, dq = T.kv_write(cache, x, pos, rope=tabs, scales=scales, deq=True)
    x64 = _rot64(x, tabs, pos)
    amax = x64.abs().amax(-1)
    for i, p in enumerate(pos.tolist()):
        sc = scales[i, p:p + S].cpu().double()
        assert bool(((sc - amax[i] / 127).abs() <= 1e-6 * sc).all())
        held = _deq(cache[i, p:p + S], scales[i, p:p + S])
        assert torch.equal(held, dq[i].cpu())
        assert bool(((held.double() - x64[i]).abs() <= (sc / 2 + 2e-6 * amax[i])[..., None]).all())


# ------------------------------------------------------------------ 3. attention over a given cache
def _attn_bar(got, q, kc, vc, ks, vs, pos, tabs=None, what=None):
    """The fp32 cache's bar on the dequantized caches: e <= max(4 e32, 2e-6) against fp64."""
    p = pos.cpu()
    kd, vd = _deq(kc, ks), _deq(vc, vs)
    ref64 = sdpa_cache_ref(_rot64(q, tabs, p), kd.double(), vd.double(), p)
    q32 = q.float().cpu()
    if tabs is not None:
        q32 = rotary_at_ref(q32, tabs[0].cpu(), tabs[1].cpu(), p)
    ref32 = sdpa_cache_ref(q32, kd, vd, p)
    also = sdpa_cache_ref(q32, kc.cpu(), vc.cpu(), p, None, ks.cpu(), vs.cpu())     # the i8 form of the reference
    assert torch.equal(also, ref32)
    e = float((got.double().cpu() - ref64).abs().max())
    e32 = float((ref32.double() - ref64).abs().max())
    print(f"{what}: e = {e:.3g}, e32 = {e32:.3g}")
    assert got.shape == ref64.shape and e <= max(4 * e32, 2e-6), (what, e, e32)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G, Sq", [(4, 1), (8, 5), (3, 11), (32, 1)])
def test_decode_attention_over_an_int8_cache(D, G, Sq):
    hkv = 1 if G == 32 else HKV
    H = G * hkv
    g = _gen(D + G + Sq)
    kc, vc, ks, vs = _caches(g, B, D, hkv)
    q = _randn(g, B, Sq, H, D) / 256            # |k| reaches 127 x 64: logits of a few tens
    pos = _pos(5, 126)                          # the second crosses a 128-key split
    for tabs in (None, _tables(L, D)):
        got = T.sdpa_cache(q, kc, vc, pos, rope=tabs, scales=(ks, vs))
        _attn_bar(got, q, kc, vc, ks, vs, pos, tabs, what=(D, G, Sq, tabs is not None))
        sync = torch.zeros(B * hkv, dtype=torch.int32, device="cuda")
        assert torch.equal(T.sdpa_cache(q, kc, vc, pos, rope=tabs, scales=(ks, vs), sync=sync), got)
        assert int(sync.abs().sum()) == 0
        if Sq == 1:     # the partials are fp32 whatever the cache: both O-projection forms combine them
            w = _randn(g, 48, H * D) / 16
            want = T.gemv(got.reshape(B, H * D), w)
            parts = T.sdpa_cache(q, kc, vc, pos, rope=tabs, scales=(ks, vs), partials=True)
            assert torch.equal(T.gemv_partials(parts, w), want)
            wq, wsc = _quant(w)
            wq, wsc = wq.cuda(), wsc.cuda()
            parts = T.sdpa_cache(q, kc, vc, pos, rope=tabs, scales=(ks, vs), partials=True)
            assert torch.equal(T.gemv_q8_partials(parts, wq, wsc), T.gemv_q8(got.reshape(B, H * D), wq, wsc))


# ------------------------------------------------------------------ 4. fresh rows
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rope", [False, True])
def test_decode_attention_quantizes_the_fresh_rows_as_kv_write_does(D, rope):
    """``fresh=``: caches and scales bit-equal to ``kv_write`` + ``sdpa_cache``, the outputs
    to fp32 round-off -- the step attends its own rows as the cache holds them."""
    G = 4
    H = G * HKV
    tabs = _tables(L, D) if rope else None
    pos = _pos(5, 126)
    for Sq in (1, 3, 20):
        g = _gen(Sq + D)
        kc, vc, ks, vs = _caches(g, B, D)
        q = _randn(g, B, Sq, H, D) / 256
        kx = (_randn(g, B, Sq, 3 * HKV, D) * 40)[:, :, :HKV]     # strided rows, as from a fused projection
        vx = _randn(g, B, Sq, HKV, D) * 40
        kc2, vc2, ks2, vs2 = kc.clone(), vc.clone(), ks.clone(), vs.clone()
        T.kv_write(kc2, kx, pos, rope=tabs, second=(vc2, vx, vs2), scales=ks2)
        ref = T.sdpa_cache(q, kc2, vc2, pos, rope=tabs, scales=(ks2, vs2))
        got = T.sdpa_cache(q, kc, vc, pos, rope=tabs, fresh=(kx, vx), scales=(ks, vs))
        torch.cuda.synchronize()
        assert torch.equal(kc, kc2) and torch.equal(vc, vc2) and torch.equal(ks, ks2) and torch.equal(vs, vs2)
        print(f"Sq = {Sq}: max |fresh - written| = {float((got - ref).abs().max()):.3g}")
        torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_of_one_fresh_key_returns_the_dequantized_value(D):
    """Position 0, one query token: the output IS the V row as the cache now holds it."""
    G = 4
    g = _gen(D)
    kc, vc, ks, vs = _caches(g, B, D)
    q = _randn(g, B, 1, G * HKV, D)
    kx, vx = _randn(g, B, 1, HKV, D), _randn(g, B, 1, HKV, D)
    got = T.sdpa_cache(q, kc, vc, _pos(0, 0), fresh=(kx, vx), scales=(ks, vs))
    qv, sv = _quant(vx)
    assert torch.equal(vc[:, :1].cpu(), qv) and torch.equal(vs[:, :1].cpu(), sv)
    want = _deq(qv, sv)[:, 0].repeat_interleave(G, dim=1)          # [B, H, D]
    assert bool((want != vx.cpu()[:, 0].repeat_interleave(G, dim=1)).float().mean() > 0.9)
    assert torch.equal(got[:, 0].cpu(), want)


# ------------------------------------------------------------------ 5. unwritten memory
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq", [1, 5])
@pytest.mark.parametrize("fill", [float("nan"), float("inf")])
def test_decode_attention_never_reads_rows_past_the_visible_keys(D, Sq, fill):
    b, G = 3, 4
    H = G * HKV
    g = _gen(D + Sq)
    kc, vc, ks, vs = _caches(g, b, D)
    q = _randn(g, b, Sq, H, D) / 256
    pos = _pos(0, 120, 250)
    zero = [t.clone() for t in (kc, vc, ks, vs)]
    bad = [t.clone() for t in (kc, vc, ks, vs)]
    for i, p in enumerate(pos.tolist()):
        for t in zero:
            t[i, p + Sq:] = 0
        bad[0][i, p + Sq:] = -128
        bad[1][i, p + Sq:] = -128
        bad[2][i, p + Sq:] = fill
        bad[3][i, p + Sq:] = fill
    want = T.sdpa_cache(q, zero[0], zero[1], pos, scales=(zero[2], zero[3]))
    got = T.sdpa_cache(q, bad[0], bad[1], pos, scales=(bad[2], bad[3]))
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    sync = torch.zeros(b * HKV, dtype=torch.int32, device="cuda")
    assert torch.equal(T.sdpa_cache(q, bad[0], bad[1], pos, scales=(bad[2], bad[3]), sync=sync), want)
    if Sq == 1:
        w = _randn(g, 48, H * D) / 16
        y = T.gemv_partials(T.sdpa_cache(q, bad[0], bad[1], pos, scales=(bad[2], bad[3]), partials=True), w)
        assert bool(torch.isfinite(y).all()) and torch.equal(y, T.gemv(want.reshape(b, H * D), w))


# ------------------------------------------------------------------ 6. bad arguments
@pytest.mark.parametrize("case", ["ok", "null-kscales", "null-vscales", "misaligned-cache", "d-96", "g-33", "nfresh"])
def test_attn_decode_q8_refuses_bad_arguments_without_a_launch(case):
    Sq, hkv, G, D, Lc = 2, 1, 4, 64, 16
    if case == "d-96":
        D = 96
    if case == "g-33":
        G = 33
    q = torch.ones(1, Sq, G, D, device="cuda")
    store = torch.ones(Lc * hkv * D + 16, dtype=I8, device="cuda")
    off = 8 if case == "misaligned-cache" else 0
    kc = store[off:off + Lc * hkv * D].view(1, Lc, hkv, D)
    vc = torch.ones(1, Lc, hkv, D, dtype=I8, device="cuda")
    ks, vs = torch.ones(1, Lc, hkv, device="cuda"), torch.ones(1, Lc, hkv, device="cuda")
    kn, vn = torch.ones(1, Sq, hkv, D, device="cuda"), torch.ones(1, Sq, hkv, D, device="cuda")
    pos = _pos(3)
    out = torch.full((1, Sq, G, D), 7.0, device="cuda")
    ws = torch.zeros(1 << 16, device="cuda")
    nfresh = Sq - 1 if case == "nfresh" else (Sq if case == "ok" else 0)
    rc = _lib.lib().nos_attn_decode_q8(
        q.data_ptr(), G * D, Sq * G * D, kc.data_ptr(), vc.data_ptr(), None if case == "null-kscales" else ks.data_ptr(),
        None if case == "null-vscales" else vs.data_ptr(), pos.data_ptr(), None, None, 0, out.data_ptr(), 1, G * hkv,
        hkv, Sq, Lc, D, 1.0 / math.sqrt(D), ws.data_ptr(), ws.numel() * 4, kn.data_ptr(), vn.data_ptr(), hkv * D,
        Sq * hkv * D, hkv * D, Sq * hkv * D, nfresh, None, 0, 0, _stream())
    torch.cuda.synchronize()
    if case == "ok":     # the same call with nothing wrong runs: the refusals below are the arguments'
        assert rc == 0 and bool((out != 7.0).all()) and int(kc[0, 3, 0, 0]) == 127
        return
    assert rc != 0 and bool((out == 7.0).all())
    assert bool((kc == 1).all()) and bool((vc == 1).all()) and bool((ks == 1).all()) and bool((vs == 1).all())


@pytest.mark.parametrize("case", ["null-scales", "misaligned-cache", "d-96", "s-over-l", "null-scales2"])
def test_kv_write_q8_refuses_bad_arguments_without_a_launch(case):
    S, H, D, Lc = 2, 2, 96 if case == "d-96" else 64, 1 if case == "s-over-l" else 16
    x, x2 = torch.ones(1, S, H, D, device="cuda"), torch.ones(1, S, H, D, device="cuda")
    store = torch.full((Lc * H * D + 16,), 77, dtype=I8, device="cuda")
    off = 4 if case == "misaligned-cache" else 0
    cache = store[off:off + Lc * H * D].view(1, Lc, H, D)
    cache2 = torch.full((1, Lc, H, D), 77, dtype=I8, device="cuda")
    sc, sc2 = torch.full((1, Lc, H), -5.0, device="cuda"), torch.full((1, Lc, H), -5.0, device="cuda")
    pos = _pos(0)
    rc = _lib.lib().nos_kv_write_q8(x.data_ptr(), H * D, S * H * D, cache.data_ptr(),
                                    None if case == "null-scales" else sc.data_ptr(), None, pos.data_ptr(), None, None,
                                    0, 1, S, H, D, Lc, x2.data_ptr(), H * D, S * H * D, cache2.data_ptr(),
                                    None if case == "null-scales2" else sc2.data_ptr(), None, _stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((store == 77).all()) and bool((cache2 == 77).all()) and bool((sc == -5).all()) and bool((sc2 == -5).all())


# ------------------------------------------------------------------ 7, 8. a tenant compiled for the GPU
@pytest.fixture(scope="module")
def model():
    from nos_amd.models.llama_program import llama_config, llama_model

    return llama_model(llama_config(False), 0)


def _compile(model, device, prompt_len=8, max_len=64, **kw):
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    progs, w = llama_decode_programs(model, prompt_len, max_len, **kw)
    ps = PG.parse_variants(progs, w, gpu=device == "cuda")
    params, state = ps[0].tensors(device), ps[0].state_tensors(device)
    return [p.compile(device, params=params, state=state) for p in ps], state


def test_int8_kv_tenant_on_the_gpu(model):
    """Prefill 8 + 3 steps against the same programs compiled for the CPU, fed the same
    tokens; both against the unquantized HF model in fp64, relative to max |ref64|:
    e_gpu <= 2 e_cpu (both quantize at the same graph edges; two for the summation
    orders and the rare value that falls to the other side of a rounding boundary).
    Measured on an MI355X: e_gpu = 6.71e-3, e_cpu = 6.71e-3 (the quantization's own error)."""
    (pre, step), state = _compile(model, "cuda", kv="int8")
    assert state["kc0"].dtype == I8 and state["vc1"].dtype == I8 and state["ks0"].dtype == F32
    prompt = torch.randint(0, model.config.vocab_size, (1, 8), generator=_gen(0))
    toks = []
    with torch.no_grad():
        logits, nxt = pre(prompt.int().cuda())
        for _ in range(3):
            toks.append(nxt.view(1, 1).int())
            logits, nxt = step(toks[-1])
    assert logits.dtype == F32 and state["pos"].tolist() == [11]
    seq = torch.cat([prompt] + [t.cpu().long() for t in toks], 1)
    (cpre, cstep), cstate = _compile(model, "cpu", kv="int8")
    with torch.no_grad():
        clogits = cpre(prompt.int())[0]
        for t in toks:
            clogits = cstep(t.cpu())[0]
        ref64 = copy.deepcopy(model).double()(seq).logits[:, -1:]
    assert cstate["pos"].tolist() == [11] and clogits.shape == ref64.shape == logits.shape
    scale = float(ref64.abs().max())
    e_gpu = float((logits.double().cpu() - ref64).abs().max()) / scale
    e_cpu = float((clogits.double() - ref64).abs().max()) / scale
    print(f"int8-KV tenant: e_gpu = {e_gpu:.3g}, e_cpu = {e_cpu:.3g}")
    assert e_gpu <= 2 * e_cpu, (e_gpu, e_cpu)
    assert state["kc0"].dtype == I8 and state["ks0"].dtype == F32
    assert bool(state["kc0"][0, :11].any()) and not bool(state["kc0"][0, 11:].any())


@pytest.mark.parametrize("weights", ["fp32", "int8"])
def test_int8_kv_step_keeps_every_fusion_of_the_fp32_step(model, weights):
    (pre, q8), _ = _compile(model, "cuda", kv="int8", weights=weights)
    (pre32, f32), _ = _compile(model, "cuda", weights=weights)
    layers = model.config.num_hidden_layers
    keys = ["kv_writes_paired", "kv_writes_into_attention", "rotary_at_fused", "gemv_glu_fused", "q8_glu_fused",
            "decode_combines_into_gemv", "q8_combines_into_gemv", "kernels"]
    for key in keys:
        assert q8.stats[key] == f32.stats[key], (key, q8.stats, f32.stats)
    assert q8.stats["kv_writes_into_attention"] == layers
    assert q8.stats["decode_combines_into_gemv"] + q8.stats["q8_combines_into_gemv"] == layers
    assert q8.stats["kv_q8_caches"] == 2 * layers and f32.stats["kv_q8_caches"] == 0
    assert "kv_write" not in [s.kind for s in q8.steps]
    assert pre.stats["static_positions"] == pre32.stats["static_positions"] == 3 * layers


def test_int8_kv_prefill_of_16_tokens_attends_the_deq_rows_with_the_flash_kernel(model):
    """Position 0 is static: ``sdpa_cache`` becomes the causal flash ``sdpa`` on the rows the
    writes hand over dequantized -- the prefill still attends what the cache holds, so the
    step after it continues the CPU programs' sequence."""
    (pre, step), state = _compile(model, "cuda", prompt_len=16, kv="int8")
    (pre32, _), _ = _compile(model, "cuda", prompt_len=16)
    layers = model.config.num_hidden_layers
    assert pre.stats["static_positions"] == pre32.stats["static_positions"] == 3 * layers
    kinds = [s.kind for s in pre.steps]
    assert kinds.count("sdpa") == layers and "sdpa_cache" not in kinds and kinds.count("kv_write") == 2 * layers
    for s in pre.steps:
        if s.kind == "sdpa":
            assert s.inputs[1].endswith("::deq") and s.inputs[2].endswith("::deq")
    prompt = torch.randint(0, model.config.vocab_size, (1, 16), generator=_gen(1))
    (cpre, cstep), cstate = _compile(model, "cpu", prompt_len=16, kv="int8")
    with torch.no_grad():
        logits, nxt = pre(prompt.int().cuda())
        clogits, cnxt = cpre(prompt.int())
        ref64 = copy.deepcopy(model).double()(prompt.long()).logits[:, -1:]
    scale = float(ref64.abs().max())
    e_gpu = float((logits.double().cpu() - ref64).abs().max()) / scale
    e_cpu = float((clogits.double() - ref64).abs().max()) / scale
    print(f"int8-KV prefill 16: e_gpu = {e_gpu:.3g}, e_cpu = {e_cpu:.3g}")
    assert e_gpu <= 2 * e_cpu, (e_gpu, e_cpu)
    assert state["pos"].tolist() == [16]
    # the bytes the GPU prefill left are the CPU prefill's, up to values at a rounding boundary: layer 0's K
    # differs between the two by ~1e-6 of its size (fp32 GEMMs in another order), a quantization step is
    # max|row| / 127, so a value flips with probability <= 2 x 1e-6 x 127 = 2.5e-4 -- and then by one step
    same =(state["kc0"].cpu() == cstate["kc0"]).float().mean()
    assert float(same) > 0.999 and int((state["kc0"].cpu().int() - cstate["kc0"].int()).abs().max()) <= 1


# ------------------------------------------------------------------ 9, 10. the server
PROMPT_LEN, NEW, MAX_LEN = 16, 16, 64
# prompt seeds whose reference clears both gaps below (asserted there), chosen on the CPU among 0 .. 7: gap
# 1.28e-2 / 8.35e-3 against a CPU-tenant deviation of 3.0e-7 / 5.4e-7.  (One value falling to the other side
# of a rounding boundary moves the logits by ~3e-4 -- seeds 0 and 6 with int8 weights show it -- which these
# gaps also clear by more than ten times.)
SERVER_SEED = {"fp32": 6, "int8": 2}


def _server_prompt(weights):
    return np.random.default_rng(SERVER_SEED[weights]).integers(0, 512, (1, PROMPT_LEN)).astype(np.int32)


def greedy_reference(hf_model, prompt):
    """Greedy decoding of the HF model in fp64 with ``kv_q8_roundtrip_cache()``, a token at a time
    after the prompt (each K / V row quantized once, as a cache stores it): tokens [1, NEW], the
    logits of every step [NEW, vocab] and the smallest top-2 gap relative to max |logit|."""
    from nos_amd.models.llama_program import kv_q8_roundtrip_cache

    m64 = copy.deepcopy(hf_model).double()
    ids = torch.from_numpy(prompt.astype(np.int64))
    toks, rows, gap = [], [], float("inf")
    with torch.no_grad():
        r = m64(ids, past_key_values=kv_q8_roundtrip_cache(), use_cache=True)
        for _ in range(NEW):
            lg = r.logits[0, -1]
            top = lg.topk(2)
            gap = min(gap, float((top.values[0] - top.values[1]) / lg.abs().max()))
            rows.append(lg)
            toks.append(int(top.indices[0]))
            r = m64(torch.tensor([[toks[-1]]]), past_key_values=r.past_key_values, use_cache=True)
    return np.array([toks]), torch.stack(rows), gap


def cpu_tenant_deviation(model, weights, prompt, toks, rows):
    """The largest deviation of the CPU tenant's logits from the reference's over the sequence
    (fed the reference's tokens), relative to max |logit| of the step."""
    (pre, step), _ = _compile(model, "cpu", prompt_len=PROMPT_LEN, max_len=MAX_LEN, kv="int8", weights=weights)
    dev = 0.0
    with torch.no_grad():
        lg = pre(torch.from_numpy(prompt))[0]
        for i in range(NEW):
            dev = max(dev, float((lg.double().view(-1) - rows[i]).abs().max() / rows[i].abs().max()))
            if i + 1 < NEW:
                lg = step(torch.tensor([[int(toks[0, i])]], dtype=torch.int32))[0]
    return dev


@pytest.mark.parametrize("weights", ["fp32", "int8"])
def test_gpu_server_generates_the_roundtrip_models_tokens(model, weights, tmp_path):
    """HIP graphs and the server loop on an int8-KV tenant (alone, and with int8 weights against
    ``dequantized_llama``): the tokens of greedy fp64 decoding with the round-trip cache, whose
    top-2 gap is >= 1e-4 of max |logit| at every step and >= 10 x the CPU tenant's largest logit
    deviation from it; a second sequence after reset() repeats the first."""
    from nos_amd.models.llama_program import dequantized_llama, llama_decode_programs
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    prompt = _server_prompt(weights)
    hf = dequantized_llama(model) if weights == "int8" else model
    want, rows, gap = greedy_reference(hf, prompt)
    dev = cpu_tenant_deviation(model, weights, prompt, want, rows)
    print(f"{weights}: top-2 gap = {gap:.3g}, CPU tenant deviation = {dev:.3g}")
    assert gap >= 1e-4 and gap >= 10 * dev, (gap, dev)
    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, kv="int8", weights=weights)
    srv = PodServer(tmp_path / "g.sock", device="cuda", lanes=2, memory_gb=40).start()
    try:
        c = PodClient(srv.path, connect_timeout_s=60)
        c.register("llm-kvq8", progs[0], w, memory_limit_gb=4, variants=progs[1:])
        ids, tm = c.generate(prompt, NEW, server_loop=True)
        assert np.array_equal(ids, want), (ids, want)
        assert tm["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
        c.reset()
        again, tm2 = c.generate(prompt, NEW, server_loop=True)
        assert np.array_equal(again, want) and tm2["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
        c.close()
    finally:
        srv.stop()


def test_gpu_server_samples_the_same_tokens_in_the_loop_and_per_request(model, tmp_path):
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, kv="int8", sampling=True)
    prompt = _server_prompt("fp32")
    kw = dict(temperature=0.8, top_k=20, top_p=0.95, seed=7)
    srv = PodServer(tmp_path / "s.sock", device="cuda", lanes=2, memory_gb=40).start()
    try:
        c = PodClient(srv.path, connect_timeout_s=60)
        c.register("llm-kvq8-s", progs[0], w, memory_limit_gb=4, variants=progs[1:])
        loop, tl = c.generate(prompt, NEW, server_loop=True, **kw)
        step, ts = c.generate(prompt, NEW, server_loop=False, **kw)
        greedy, _ = c.generate(prompt, NEW)
        assert np.array_equal(loop, step) and not np.array_equal(loop, greedy)
        assert tl["state"] == ts["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
        c.close()
    finally:
        srv.stop()
