"""Sliding-window attention on ring K / V caches on the GPU (csrc/hip/decode.hip: ``kv_write_ring_kernel``,
``kv_write_q8_ring_kernel``, ``attn_decode_kernel<D, CBF, true>``; csrc/hip/kv_ring.h) and a compiled Mistral
tenant.

The attention oracle is banded attention in fp64 over the full K / V history the test keeps itself, as a cache of
that kind holds it (int8: through ``quantize_kv_rows`` / ``dequantize_kv_rows``; bf16: rounded), never the ring
reference; the bar is ``tests/test_decode_paths_gpu.py::_attn_bar``'s, e <= max(4 e32, 2e-6) absolute, e32 the
same oracle in fp32.  Inputs are drawn on the CPU from seeded generators."""
from __future__ import annotations

import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402
from nos_amd.ops import tenant as T  # noqa: E402
from nos_amd.podserver.program.reference import (dequantize_kv_rows, kv_write_ref, quantize_kv_rows,  # noqa: E402
                                                 rotary_at_ref)

F32, BF16, I8 = torch.float32, torch.bfloat16, torch.int8
KINDS = ["fp32", "bf16", "int8"]
CDT = {"fp32": F32, "bf16": BF16, "int8": I8}


@pytest.fixture(autouse=True)
def _h3():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _pos(*v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _tables(n, d):
    inv = 1.0 / 10000 ** (torch.arange(0, d, 2, dtype=torch.float64) / d)
    f = torch.outer(torch.arange(n, dtype=torch.float64), inv)
    e = torch.cat([f, f], 1)
    return e.cos().float().cuda(), e.sin().float().cuda()


def _rot64(x, tabs, pos):
    """``rotary_at_ref`` in fp64 (on the fp32 tables' values)."""
    if tabs is None:
        return x.double().cpu()
    B, S, H, D = x.shape
    c, s = tabs[0].double().cpu(), tabs[1].double().cpu()
    idx = (pos.cpu().long().view(B, 1) + torch.arange(S).view(1, S)).clamp(0, c.shape[0] - 1)
    xd = x.double().cpu()
    rot = torch.cat([-xd[..., D // 2:], xd[..., :D // 2]], dim=-1)
    return xd * c[idx][:, :, None, :] + rot * s[idx][:, :, None, :]


def held(s, pmax, C):
    return pmax - ((pmax - s) % C)


def visible(s, qpos, pmax, C, W):
    a = held(s, pmax, C)
    return a >= 0 and a <= qpos and a > qpos - W


# ------------------------------------------------------------------ 1. the ring writes
WB, WHKV, WD, WC, WS, WLIMIT = 2, 2, 64, 12, 3, 40
WPOS = (10, 23)          # 10, 11 | 0: wraps inside the launch; 23 | 0, 1


def _write_state(kind, fill):
    cache = torch.full((WB, WC, WHKV, WD), fill, dtype=F32).to(CDT[kind]).cuda()
    scales = torch.full((WB, WC, WHKV), -5.0, device="cuda") if kind == "int8" else None
    return cache, scales


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_ring_writes_put_every_row_in_its_slot(kind, rope):
    """K (rotated or not) and V in one launch, and K alone, against the CPU reference at the plain writes' bars
    (no rotation: bit equality; rotated: 1e-6 fp32, 1e-2 bf16, for int8 the scale to 1e-6 and every value within
    half a step of the fp64 rotation); every slot not written keeps its bits; ``deq`` is what the cache holds."""
    g = _gen(len(kind) + rope)
    xdt = BF16 if kind == "bf16" else F32
    x, x2 = (torch.randn(WB, WS, WHKV, WD, generator=g).to(xdt).cuda() for _ in range(2))
    pos = _pos(*WPOS)
    tabs = _tables(WLIMIT, WD) if rope else None
    kw = dict(window=8, limit=WLIMIT)
    cache, scales = _write_state(kind, 77)
    cache2, scales2 = _write_state(kind, 77)
    written = torch.zeros(WB, WC, dtype=torch.bool)
    for b, p in enumerate(WPOS):
        written[b, [(p + i) % WC for i in range(WS)]] = True
    if kind == "int8":
        got, dq, dq2 = T.kv_write(cache, x, pos, rope=tabs, second=(cache2, x2, scales2), scales=scales, deq=True, **kw)
    else:
        got = T.kv_write(cache, x, pos, rope=tabs, second=(cache2, x2), **kw)
    torch.cuda.synchronize()
    assert got is cache
    # the reference, on the CPU (K rotated there)
    rc, rs = _write_state(kind, 77)
    rc2, rs2 = _write_state(kind, 77)
    xr = rotary_at_ref(x.cpu(), tabs[0].cpu(), tabs[1].cpu(), pos.cpu()) if rope else x.cpu()
    rc, rc2 = rc.cpu(), rc2.cpu()
    rs, rs2 = (None, None) if rs is None else (rs.cpu(), rs2.cpu())
    kv_write_ref(rc, xr, pos.cpu(), rs, **kw)
    kv_write_ref(rc2, x2.cpu(), pos.cpu(), rs2, **kw)
    assert torch.equal(cache2.cpu(), rc2) and (kind != "int8" or torch.equal(scales2.cpu(), rs2))     # V: never rotated
    for c, s in ((cache, scales), (cache2, scales2)):
        assert bool((c.cpu()[~written].float() == 77).all()) and (s is None or bool((s.cpu()[~written] == -5.0).all()))
    if not rope:
        assert torch.equal(cache.cpu(), rc) and (kind != "int8" or torch.equal(scales.cpu(), rs))
    elif kind != "int8":
        tol = 1e-6 if kind == "fp32" else 1e-2
        torch.testing.assert_close(cache.cpu().float(), rc.float(), rtol=tol, atol=tol)
    else:
        x64 = _rot64(x, tabs, pos)
        amax = x64.abs().amax(-1)
        for b, p in enumerate(WPOS):
            slots = [(p + i) % WC for i in range(WS)]
            sc = scales[b, slots].cpu().double()
            assert bool(((sc - amax[b] / 127).abs() <= 1e-6 * sc).all())
            have = dequantize_kv_rows(cache[b, slots].cpu(), scales[b, slots].cpu())
            assert bool(((have.double() - x64[b]).abs() <= (sc / 2 + 2e-6 * amax[b])[..., None]).all())
    if kind == "int8":
        for b, p in enumerate(WPOS):
            slots = [(p + i) % WC for i in range(WS)]
            assert torch.equal(dq[b].cpu(), dequantize_kv_rows(cache[b, slots].cpu(), scales[b, slots].cpu()))
            assert torch.equal(dq2[b].cpu(), dequantize_kv_rows(cache2[b, slots].cpu(), scales2[b, slots].cpu()))
    # a single write is the pair's first half
    c1, s1 = _write_state(kind, 77)
    assert T.kv_write(c1, x, pos, rope=tabs, scales=s1, **kw) is c1
    assert torch.equal(c1, cache) and (s1 is None or torch.equal(s1, scales))


@pytest.mark.parametrize("kind", KINDS)
def test_ring_writes_drop_rows_outside_the_limit(kind):
    """A row at position -1 and a row at position ``limit`` leave caches and scales bit-unchanged; the rows
    beside them land (``ring_slot`` returns -1 before any address is formed: tests/test_window.py)."""
    g = _gen(7)
    xdt = BF16 if kind == "bf16" else F32
    x = torch.randn(2, 1, WHKV, WD, generator=g).to(xdt).cuda()
    for rope in (None, _tables(WLIMIT, WD)):
        cache, scales = _write_state(kind, 77)
        cache2, scales2 = _write_state(kind, 77)
        sec = (cache2, x, scales2) if kind == "int8" else (cache2, x)
        T.kv_write(cache, x, _pos(-1, WLIMIT), rope=rope, second=sec, scales=scales, window=8, limit=WLIMIT)
        torch.cuda.synchronize()
        for c, s in ((cache, scales), (cache2, scales2)):
            assert bool((c.float() == 77).all()) and (s is None or bool((s == -5.0).all()))
        x3 = torch.randn(2, 3, WHKV, WD, generator=g).to(xdt).cuda()
        T.kv_write(cache, x3, _pos(-1, WLIMIT - 2), rope=rope, scales=scales, window=8, limit=WLIMIT)
        torch.cuda.synchronize()
        hit = torch.zeros(2, WC, dtype=torch.bool)
        hit[0, [0, 1]] = True                                       # positions 0, 1 of the row that starts at -1
        hit[1, [(WLIMIT - 2) % WC, (WLIMIT - 1) % WC]] = True       # positions limit - 2, limit - 1; limit dropped
        assert bool((cache.cpu()[~hit].float() == 77).all()) and bool((cache.cpu()[hit].float() != 77).any(-1).all())


# ------------------------------------------------------------------ 2. the ring attention
def banded(q, kh, vh, p0, W, scale, dt):
    """q [Sq, H, D] at positions p0 + i over the full history kh / vh [T, Hkv, D], in ``dt``."""
    Sq, H, D = q.shape
    G = H // kh.shape[1]
    out = torch.zeros(Sq, H, D, dtype=dt)
    for i in range(Sq):
        p = p0 + i
        lo = max(0, p - W + 1)
        k = kh[lo:p + 1].to(dt).repeat_interleave(G, dim=1)
        v = vh[lo:p + 1].to(dt).repeat_interleave(G, dim=1)
        s = torch.einsum("hd,khd->hk", q[i].to(dt), k) * scale
        out[i] = torch.einsum("hk,khd->hd", torch.softmax(s, -1), v)
    return out


def _as_cache(x, kind):
    if kind == "int8":
        return dequantize_kv_rows(*quantize_kv_rows(x))
    return x.to(BF16).float() if kind == "bf16" else x


def _ring_state(kind, hist, upto, C, fill=7.0):
    """Ring caches (and scales) on the GPU holding the positions < upto[b] of ``hist`` [B, T, Hkv, D], the
    slots never written filled with ``fill``."""
    B, _, Hkv, D = hist.shape
    c = torch.full((B, C, Hkv, D), fill).to(CDT[kind])
    s = torch.full((B, C, Hkv), 0.5) if kind == "int8" else None
    for b in range(B):
        for p in range(max(0, upto[b] - C), upto[b]):
            if kind == "int8":
                c[b, p % C], s[b, p % C] = quantize_kv_rows(hist[b, p])
            else:
                c[b, p % C] = hist[b, p].to(CDT[kind])
    return c.cuda(), (s.cuda() if s is not None else None)


CASES = {
    "one-split-wraps": dict(W=8, C=8, Sq=1, G=2, D=64, pos=(0, 7, 8, 21)),
    "two-splits": dict(W=193, C=200, Sq=8, G=4, D=128, pos=(150, 196, 700)),
    "two-launches": dict(W=40, C=47, Sq=8, G=8, D=64, pos=(100, 30)),
    "w1": dict(W=1, C=1, Sq=1, G=2, D=64, pos=(0, 5)),
    "w1-steps-of-3": dict(W=1, C=3, Sq=3, G=2, D=64, pos=(0, 4)),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_ring_attention_is_banded_attention(name, kind):
    """Every case against the fp64 oracle at the bar, with a last sequence at position -1 (zero rows); the plain
    call, the ``fresh`` form (rotated too), the ``sync`` form and the partials into ``gemv_partials`` agree bit
    for bit; NaN in every slot (and scale) no query row of the step sees changes no bit; a rerun is identical."""
    cs = CASES[name]
    W, C, Sq, G, D = cs["W"], cs["C"], cs["Sq"], cs["G"], cs["D"]
    pos_l = list(cs["pos"]) + [-1]
    B, Hkv = len(pos_l), 2
    H = G * Hkv
    T_ = max(pos_l) + Sq
    limit = T_ + 3
    g = _gen(len(name) + len(kind))
    kh, vh = torch.randn(B, T_, Hkv, D, generator=g), torch.randn(B, T_, Hkv, D, generator=g)
    qdt = F32            # fp32 activations over every cache kind; a bf16 q is the fp32 call rounded once (below)
    q = (torch.randn(B, Sq, H, D, generator=g) / 2).to(BF16).float()
    scale = 1 / math.sqrt(D)
    pos = _pos(*pos_l)
    kw = dict(window=W, limit=limit, scale=scale)
    good = [max(p, 0) for p in pos_l]

    def caches(upto_extra):
        kc, ks = _ring_state(kind, kh, [p + upto_extra for p in good], C)
        vc, vs = _ring_state(kind, vh, [p + upto_extra for p in good], C)
        return kc, vc, ((ks, vs) if kind == "int8" else None)

    # the step's rows written by the ring write kernel, then the plain call
    kc, vc, sc = caches(0)
    step = lambda h: torch.stack([h[b, good[b]:good[b] + Sq] for b in range(B)]).to(qdt).cuda()  # noqa: E731
    kn, vn = step(kh), step(vh)
    if kind == "int8":
        T.kv_write(kc, kn, pos, second=(vc, vn, sc[1]), scales=sc[0], window=W, limit=limit)
    else:
        T.kv_write(kc, kn, pos, second=(vc, vn), window=W, limit=limit)
    got = T.sdpa_cache(q.cuda(), kc, vc, pos, scales=sc, **kw)
    torch.cuda.synchronize()
    assert got.dtype == qdt and not bool(got[-1].any())
    e = e32 = 0.0
    for b in range(B - 1):
        hk, hv = _as_cache(kh[b], kind), _as_cache(vh[b], kind)
        r64 = banded(q[b].float(), hk, hv, pos_l[b], W, scale, torch.float64)
        r32 = banded(q[b].float(), hk, hv, pos_l[b], W, scale, F32)
        e = max(e, float((got[b].double().cpu() - r64).abs().max()))
        e32 = max(e32, float((r32.double() - r64).abs().max()))
    print(f"{name} {kind}: e = {e:.3g}, e32 = {e32:.3g}")
    assert e <= max(4 * e32, 2e-6), (name, kind, e, e32)
    # a rerun, and the combine in the launch's last workgroup
    assert torch.equal(T.sdpa_cache(q.cuda(), kc, vc, pos, scales=sc, **kw), got)
    sync = torch.zeros(B * Hkv, dtype=torch.int32, device="cuda")
    assert torch.equal(T.sdpa_cache(q.cuda(), kc, vc, pos, scales=sc, sync=sync, **kw), got)
    assert int(sync.abs().sum()) == 0
    # the fresh form: the launch writes the step's rows itself, into the same slots with the same bits
    fk, fv, fs = caches(0)
    out = T.sdpa_cache(q.cuda(), fk, fv, pos, scales=fs, fresh=(kn, vn), **kw)
    # (the sequence at -1: the write kernel keeps its rows at positions >= 0, the attention writes none of them)
    assert torch.equal(out, got) and torch.equal(fk[:-1], kc[:-1]) and torch.equal(fv[:-1], vc[:-1])
    assert fs is None or (torch.equal(fs[0][:-1], sc[0][:-1]) and torch.equal(fs[1][:-1], sc[1][:-1]))
    fk, fv, fs = caches(0)
    sync = torch.zeros(B * Hkv, dtype=torch.int32, device="cuda")
    assert torch.equal(T.sdpa_cache(q.cuda(), fk, fv, pos, scales=fs, fresh=(kn, vn), sync=sync, **kw), got)
    assert int(sync.abs().sum()) == 0 and torch.equal(fk[:-1], kc[:-1])
    if kind == "bf16":   # bf16 activations: the same fp32 arithmetic, the result rounded once
        assert torch.equal(T.sdpa_cache(q.cuda().bfloat16(), kc, vc, pos, **kw), got.bfloat16())
    # the partials into the O-projection GEMV (one fp32 query token)
    if Sq == 1:
        w = (torch.randn(48, H * D, generator=g) / 16).cuda()
        want = T.gemv(got.reshape(B, H * D), w)
        parts = T.sdpa_cache(q.cuda(), kc, vc, pos, scales=sc, partials=True, **kw)
        assert parts.NS == (C + 127) // 128 and torch.equal(T.gemv_partials(parts, w), want)
        fk, fv, fs = caches(0)
        parts = T.sdpa_cache(q.cuda(), fk, fv, pos, scales=fs, fresh=(kn, vn), partials=True, **kw)
        assert torch.equal(T.gemv_partials(parts, w), want)
    # NaN (int8: the scale, and bytes of 127) in every slot no query row of the step sees
    pk, pv = kc.clone(), vc.clone()
    ps = None if sc is None else (sc[0].clone(), sc[1].clone())
    hidden = 0
    for b in range(B):
        pmax = pos_l[b] + Sq - 1
        for s in range(C):
            if pos_l[b] < 0 or not any(visible(s, pos_l[b] + i, pmax, C, W) for i in range(Sq)):
                hidden += 1
                for t in (pk, pv):
                    t[b, s] = 127 if kind == "int8" else float("nan")
                if ps is not None:
                    ps[0][b, s] = ps[1][b, s] = float("nan")
    assert hidden >= C                   # the sequence at -1 at least
    bad = T.sdpa_cache(q.cuda(), pk, pv, pos, scales=ps, **kw)
    assert bool(torch.isfinite(bad.float()).all()) and torch.equal(bad, got)


@pytest.mark.parametrize("kind", KINDS)
def test_ring_attention_with_rope_and_fresh_rows_is_write_then_attend(kind):
    """Rotary on q and on the fresh K inside the launch, two splits with the wrap inside the fresh rows: equal, bit
    for bit, to the ring write (rotating K) followed by the attention (rotating q), and at the bar against banded
    attention, q rotated in fp64, over the history the caches hold (the rotating write is held to the CPU
    reference by ``test_ring_writes_put_every_row_in_its_slot``)."""
    W, C, Sq, G, D, Hkv = 193, 200, 8, 4, 128, 2
    pos_l = [196, 150]
    B, H = 2, G * Hkv
    limit = 230
    tabs = _tables(limit, D)
    g = _gen(3 + len(kind))
    qdt = F32
    kraw, vh = torch.randn(B, limit, Hkv, D, generator=g), torch.randn(B, limit, Hkv, D, generator=g)
    q = torch.randn(B, Sq, H, D, generator=g) / 2
    zero = torch.zeros(B, dtype=torch.int32)
    assert W + Sq - 1 <= C          # the positions older than pmax - C + 1 lie outside every window of the step
    kh = rotary_at_ref(kraw, tabs[0].cpu(), tabs[1].cpu(), zero)         # the history as the caches hold it: rotated
    pos = _pos(*pos_l)
    kw = dict(window=W, limit=limit, rope=tabs)

    def caches():
        kc, ks = _ring_state(kind, kh, pos_l, C)
        vc, vs = _ring_state(kind, vh, pos_l, C)
        return kc, vc, ((ks, vs) if kind == "int8" else None)

    kn = torch.stack([kraw[b, p:p + Sq] for b, p in enumerate(pos_l)]).to(qdt).cuda()
    vn = torch.stack([vh[b, p:p + Sq] for b, p in enumerate(pos_l)]).to(qdt).cuda()
    kc, vc, sc = caches()
    if kind == "int8":
        T.kv_write(kc, kn, pos, rope=tabs, second=(vc, vn, sc[1]), scales=sc[0], window=W, limit=limit)
    else:
        T.kv_write(kc, kn, pos, rope=tabs, second=(vc, vn), window=W, limit=limit)
    want = T.sdpa_cache(q.cuda(), kc, vc, pos, scales=sc, **kw)
    fk, fv, fs = caches()
    got = T.sdpa_cache(q.cuda(), fk, fv, pos, scales=fs, fresh=(kn, vn), **kw)
    assert torch.equal(got, want) and torch.equal(fk, kc) and torch.equal(fv, vc)
    assert fs is None or (torch.equal(fs[0], sc[0]) and torch.equal(fs[1], sc[1]))
    q64 = _rot64(q, tabs, pos)
    q32 = rotary_at_ref(q, tabs[0].cpu(), tabs[1].cpu(), pos.cpu())
    e = e32 = 0.0
    for b in range(B):
        pmax = pos_l[b] + Sq - 1
        hk, hv = torch.zeros(pmax + 1, Hkv, D), torch.zeros(pmax + 1, Hkv, D)
        for p in range(max(0, pmax - C + 1), pmax + 1):       # what the caches hold, by position
            if kind == "int8":
                hk[p] = dequantize_kv_rows(kc[b, p % C].cpu(), sc[0][b, p % C].cpu())
                hv[p] = dequantize_kv_rows(vc[b, p % C].cpu(), sc[1][b, p % C].cpu())
            else:
                hk[p], hv[p] = kc[b, p % C].float().cpu(), vc[b, p % C].float().cpu()
        r64 = banded(q64[b], hk, hv, pos_l[b], W, 1 / math.sqrt(D), torch.float64)
        r32 = banded(q32[b], hk, hv, pos_l[b], W, 1 / math.sqrt(D), F32)
        e = max(e, float((got[b].double().cpu() - r64).abs().max()))
        e32 = max(e32, float((r32.double() - r64).abs().max()))
    print(f"rope fresh {kind}: e = {e:.3g}, e32 = {e32:.3g}")
    assert e <= max(4 * e32, 2e-6), (kind, e, e32)


@pytest.mark.parametrize("Sq", [1, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_ring_kernel_is_the_plain_kernel_where_the_window_hides_nothing(kind, Sq):
    """C == L = 200, W = 200, position 100: nothing hidden, nothing wrapped -- the ring kernel's output is the
    plain kernel's, bit for bit (with and without fresh rows and rope)."""
    L, D, G, Hkv, B = 200, 128, 4, 2, 2
    H = G * Hkv
    g = _gen(Sq + len(kind))
    hist_k, hist_v = torch.randn(B, L, Hkv, D, generator=g), torch.randn(B, L, Hkv, D, generator=g)
    qdt = BF16 if kind == "bf16" else F32
    q = (torch.randn(B, Sq, H, D, generator=g) / 2).to(qdt).cuda()
    pos_l = [100, 100 - Sq]
    assert max(pos_l) + Sq <= L
    pos = _pos(*pos_l)
    tabs = _tables(L, D)

    def caches(extra):
        kc, ks = _ring_state(kind, hist_k, [p + extra for p in pos_l], L, fill=0.0)
        vc, vs = _ring_state(kind, hist_v, [p + extra for p in pos_l], L, fill=0.0)
        return kc, vc, ((ks, vs) if kind == "int8" else None)

    kc, vc, sc = caches(Sq)
    plain = T.sdpa_cache(q, kc, vc, pos, scales=sc)
    assert torch.equal(T.sdpa_cache(q, kc, vc, pos, scales=sc, window=L, limit=L), plain)
    assert torch.equal(T.sdpa_cache(q, kc, vc, pos, scales=sc, rope=tabs, window=L, limit=L),
                       T.sdpa_cache(q, kc, vc, pos, scales=sc, rope=tabs))
    kn = torch.stack([hist_k[b, p:p + Sq] for b, p in enumerate(pos_l)]).to(qdt).cuda()
    vn = torch.stack([hist_v[b, p:p + Sq] for b, p in enumerate(pos_l)]).to(qdt).cuda()
    a, b_ = caches(0), caches(0)
    pa = T.sdpa_cache(q, a[0], a[1], pos, scales=a[2], rope=tabs, fresh=(kn, vn))
    pb = T.sdpa_cache(q, b_[0], b_[1], pos, scales=b_[2], rope=tabs, fresh=(kn, vn), window=L, limit=L)
    assert torch.equal(pa, pb) and torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])


# ------------------------------------------------------------------ 3. a compiled tenant
MAX_LEN = 48


@pytest.fixture(scope="module")
def model():
    from nos_amd.models.llama_program import mistral_config, mistral_model

    return mistral_model(mistral_config(num_attention_heads=4, num_key_value_heads=2), 0)      # head_dim 64


def _compile(model, device, prompt_len=5, **kw):
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    progs, w = llama_decode_programs(model, prompt_len, MAX_LEN, **kw)
    ps = PG.parse_variants(progs, w, gpu=device == "cuda")
    params, state = ps[0].tensors(device), ps[0].state_tensors(device)
    return {p.inputs[0].shape[1]: p.compile(device, params=params, state=state) for p in ps}, state


def _feed(by_len, ids, plan, device):
    out, t = [], 0
    with torch.no_grad():
        for n in plan:
            out.append(by_len[n](ids[:, t:t + n].to(device))[0].cpu())
            t += n
    return torch.cat(out, 1)


def test_windowed_mistral_tenant_on_the_gpu(model):
    """Prefill 5, extend 4, 24 one-token steps (the ring of 12 slots wraps twice) on teacher-forced ids: every
    chunk's last logits against ``MistralForCausalLM`` in fp64 at the tenants' fp32 logit bar, e <= max(4 e32, 1e-5)
    relative to max |ref64| (tests/test_decode_gpu.py); the step keeps the plain tenant's launches."""
    plan = [5, 4] + [1] * 24
    ids = torch.randint(0, 512, (1, sum(plan)), generator=_gen(11), dtype=torch.int32)
    comp, state = _compile(model, "cuda", extend=(4,))
    assert state["kc0"].shape == (1, 12, 2, 64)
    got = _feed(comp, ids, plan, "cuda")
    assert state["pos"].tolist() == [sum(plan)]
    rows = (np.cumsum(plan) - 1).tolist()
    with torch.no_grad():
        r64 = copy.deepcopy(model).double()(ids.long()).logits[:, rows]
        r32 = model(ids.long()).logits[:, rows]
    scale = float(r64.abs().max())
    e = float((got.double() - r64).abs().max()) / scale
    e32 = float((r32.double() - r64).abs().max()) / scale
    print(f"windowed mistral: e = {e:.3g}, e32 = {e32:.3g}")
    assert e <= max(4 * e32, 1e-5), (e, e32)
    twin = copy.deepcopy(model)
    twin.config.sliding_window = None
    plain, _ = _compile(twin, "cuda", extend=(4,))
    layers = model.config.num_hidden_layers
    step, pstep = comp[1], plain[1]
    assert step.stats["ring_caches"] == 2 * layers and pstep.stats["ring_caches"] == 0
    for key in ("kernels", "kv_writes_paired", "kv_writes_into_attention", "rotary_at_fused", "gemv_glu_fused",
                "decode_combines_into_gemv"):
        assert step.stats[key] == pstep.stats[key], (key, step.stats, pstep.stats)
    assert step.stats["kernels"] == 5 * layers + 3          # 43 for the fleet decoder's 8 layers
    assert comp[5].stats["static_positions"] == plain[5].stats["static_positions"] == 3 * layers
    assert comp[4].stats["kernels"] == plain[4].stats["kernels"] and comp[5].stats["kernels"] == plain[5].stats["kernels"]
    for s in step.steps:
        if s.kind == "sdpa_cache":
            assert s.attrs["window"] == 8 and s.attrs["limit"] == MAX_LEN and s.attrs["fresh"] and s.attrs["partials"]


def test_gpu_server_generates_transformers_tokens(model, tmp_path):
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    prompt = np.random.default_rng(4).integers(0, 512, (1, 5)).astype(np.int32)
    with torch.no_grad():
        want = model.generate(torch.from_numpy(prompt).long(), max_new_tokens=30, do_sample=False,
                              pad_token_id=0)[:, 5:].numpy()
        ids = torch.from_numpy(np.concatenate([prompt, want], 1))
        rows = list(range(4, 34))
        r64 = copy.deepcopy(model).double()(ids.long()).logits[:, rows]
        r32 = model(ids.long()).logits[:, rows]
    top = r64.topk(2, dim=-1).values
    err = (r32.double() - r64).abs().amax(-1)
    assert bool((top[..., 0] - top[..., 1] > 4 * err).all()), "a near-tie in the reference"
    assert np.array_equal(r64.argmax(-1).numpy(), want)
    progs, w = llama_decode_programs(model, 5, MAX_LEN)
    srv = PodServer(tmp_path / "g.sock", device="cuda", lanes=2, memory_gb=40).start()
    try:
        c = PodClient(srv.path, connect_timeout_s=60)
        c.register("swa", progs[0], w, memory_limit_gb=4, variants=progs[1:])
        got, tm = c.generate(prompt, 30, server_loop=True)
        assert np.array_equal(got, want), (got, want)
        assert tm["state"] == {"pos": [34]}
        c.reset()
        assert np.array_equal(c.generate(prompt, 30, server_loop=False)[0], want)
        c.close()
    finally:
        srv.stop()


def _cpu_vs_gpu(model, ref64_model, kw, what):
    """The existing contract of the int8 and bf16 tenants: the GPU's error against the fp64 model is at most twice
    that of the same programs compiled for the CPU, fed the same tokens."""
    plan = [5] + [1] * 16
    ids = torch.randint(0, 512, (1, sum(plan)), generator=_gen(12), dtype=torch.int32)
    gpu, gstate = _compile(model, "cuda", **kw)
    cpu, cstate = _compile(model, "cpu", **kw)
    got, cgot = _feed(gpu, ids, plan, "cuda"), _feed(cpu, ids, plan, "cpu")
    assert gstate["pos"].tolist() == cstate["pos"].tolist() == [sum(plan)]
    rows = (np.cumsum(plan) - 1).tolist()
    with torch.no_grad():
        r64 = ref64_model.double()(ids.long()).logits[:, rows]
    scale = float(r64.abs().max())
    e_gpu = float((got.double() - r64).abs().max()) / scale
    e_cpu = float((cgot.double() - r64).abs().max()) / scale
    print(f"{what}: e_gpu = {e_gpu:.3g}, e_cpu = {e_cpu:.3g}")
    assert e_gpu <= 2 * e_cpu, (what, e_gpu, e_cpu)
    return gpu, gstate


def test_int8_windowed_tenant_on_the_gpu(model):
    from nos_amd.models.llama_program import dequantized_llama

    gpu, state = _cpu_vs_gpu(model, dequantized_llama(model), dict(weights="int8", kv="int8"), "int8 weights + kv, windowed")
    assert state["kc0"].dtype == I8 and state["ks0"].shape == (1, 12, 2)
    assert gpu[1].stats["ring_caches"] == gpu[1].stats["kv_q8_caches"] == 4
    assert gpu[1].stats["q8_combines_into_gemv"] == model.config.num_hidden_layers


def test_bf16_windowed_tenant_on_the_gpu(model):
    m64 = copy.deepcopy(model)
    with torch.no_grad():
        for p in m64.parameters():
            p.copy_(p.bfloat16().float())
    gpu, state = _cpu_vs_gpu(model, m64, dict(dtype="bf16"), "bf16, windowed")
    assert state["kc0"].dtype == BF16 and state["kc0"].shape == (1, 12, 2, 64)
    assert gpu[1].stats["kv_writes_into_attention"] == model.config.num_hidden_layers
