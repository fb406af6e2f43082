"""The h3 flash attention over K / V caches (csrc/hip/attention_h3g.hip ``nos_attn_h3g_cache`` /
``nos_attn_h3g_cache_ring``; ``T.sdpa_cache(flash=True)``): a multi-token step at device-side positions over
plain and ring caches, against ``sdpa_cache_ref`` in fp64.

The yardstick is the project's for the h3 kernels (tests/test_tenant_ops_gpu.py ``_close_to_fp64``): the error
against fp64 is at most max(4 x the fp32 path's error, 5e-6), the fp32 path being ``sdpa_cache(flash=False)``
(the decode kernel) on the same inputs.  Tiles are 32 keys and workgroups 256 query rows: the shapes are the
smallest with a partial tile, a diagonal inside a tile, more than one workgroup and counters that differ per
sequence."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402
from nos_amd.ops import _lib  # noqa: E402
from nos_amd.ops import tenant as T  # noqa: E402
from nos_amd.podserver.program.reference import sdpa_cache_ref  # noqa: E402

INVALID = 1   # hipErrorInvalidValue


@pytest.fixture(autouse=True)
def _config():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)
    ops.set_cu_budget(0)
    T.set_attention_h3g_kvsplit(0)


def _err(got: torch.Tensor, ref64: torch.Tensor) -> float:
    return float((got.double() - ref64).abs().max() / ref64.abs().max().clamp_min(1e-30))


def _close_to_fp64(got, ref64, fp32_got, floor=5e-6, mult=4.0):
    assert bool(torch.isfinite(got).all()), "non-finite output"
    e, e32 = _err(got.cpu(), ref64), _err(fp32_got.cpu(), ref64)
    print(f"flash err {e:.3g}, fp32 path err {e32:.3g}")
    assert e <= max(mult * e32, floor), f"flash err {e:.3g} vs fp32 path err {e32:.3g}"
    return e, e32


def _tables64(n, d):
    inv = 1.0 / 10000 ** (torch.arange(0, d, 2, dtype=torch.float64) / d)
    f = torch.outer(torch.arange(n, dtype=torch.float64), inv)
    e = torch.cat([f, f], 1)
    return e.cos(), e.sin()


def _rotate64(x, cos, sin, pos):
    """rotary_at_ref in fp64 (table rows clamped)."""
    B, S, H, D = x.shape
    idx = (pos.long().view(B, 1) + torch.arange(S).view(1, S)).clamp(0, cos.shape[0] - 1)
    c, s = cos[idx][:, :, None, :], sin[idx][:, :, None, :]
    xd = x.double()
    return xd * c + torch.cat([-xd[..., D // 2:], xd[..., :D // 2]], -1) * s


def _ref64(q, kc, vc, pos, tabs64=None, **kw):
    qd = q.double().cpu()
    if tabs64 is not None:
        qd = _rotate64(qd, tabs64[0], tabs64[1], pos.cpu())
    return sdpa_cache_ref(qd, kc.double().cpu(), vc.double().cpu(), pos.cpu(), **kw)


def _pos(*p):
    return torch.tensor(p, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------ plain caches
L = 300


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H, Hkv", [(4, 2), (8, 1)])
@pytest.mark.parametrize("Sq", [33, 40, 290])
@pytest.mark.parametrize("p", [(0, 7), (31, 64), (10, 260)])
@pytest.mark.parametrize("rope", [False, True])
def test_flash_over_plain_caches_matches_fp64(D, H, Hkv, Sq, p, rope):
    """Counters that differ per sequence, a diagonal inside a tile, rows past the cache (pos + Sq > L: they see
    every key) and, at (10, 260), one sequence with pos + Sq == L (Sq 290: the first, Sq 40: the second).  The
    cache rows at and past pos + Sq filled with 1e30 leave every bit of the result where it was: the pre-pass
    (the scales) and the kernel are bounded by the counter."""
    g = torch.Generator(device="cuda").manual_seed(D + H + Sq + p[1])
    B = 2
    kc = torch.randn(B, L, Hkv, D, device="cuda", generator=g)
    vc = torch.randn(B, L, Hkv, D, device="cuda", generator=g)
    q = torch.randn(B, Sq, H, D, device="cuda", generator=g)
    pos = _pos(*p)
    t64 = _tables64(L + Sq, D) if rope else None
    tabs = tuple(t.float().cuda() for t in t64) if rope else None
    got = T.sdpa_cache(q, kc, vc, pos, rope=tabs, flash=True)
    f32 = T.sdpa_cache(q, kc, vc, pos, rope=tabs, flash=False)
    _close_to_fp64(got, _ref64(q, kc, vc, pos, t64), f32)
    kp, vp = kc.clone(), vc.clone()
    for b in range(B):
        kp[b, p[b] + Sq:] = 1e30
        vp[b, p[b] + Sq:] = 1e30
    assert torch.equal(T.sdpa_cache(q, kp, vp, pos, rope=tabs, flash=True), got)


@pytest.mark.parametrize("rope", [False, True])
def test_flash_writes_the_fresh_rows_as_kv_write_does(rope):
    B, Hkv, H, D, Sq = 2, 2, 4, 128, 40
    g = torch.Generator(device="cuda").manual_seed(5)
    kc = torch.randn(B, L, Hkv, D, device="cuda", generator=g)
    vc = torch.randn(B, L, Hkv, D, device="cuda", generator=g)
    q = torch.randn(B, Sq, H, D, device="cuda", generator=g)
    kx = torch.randn(B, Sq, 3 * Hkv, D, device="cuda", generator=g)[:, :, :Hkv]   # strided, as from a fused projection
    vx = torch.randn(B, Sq, Hkv, D, device="cuda", generator=g)
    pos = _pos(5, 270)      # the second sequence's last rows fall off the cache
    tabs = tuple(t.float().cuda() for t in _tables64(L + Sq, D)) if rope else None
    k2, v2 = kc.clone(), vc.clone()
    T.kv_write(k2, kx, pos, rope=tabs, second=(v2, vx))
    want = T.sdpa_cache(q, k2, v2, pos, rope=tabs, flash=True)
    got = T.sdpa_cache(q, kc, vc, pos, rope=tabs, fresh=(kx, vx), flash=True)
    assert torch.equal(kc, k2) and torch.equal(vc, v2) and torch.equal(got, want)


# ------------------------------------------------------------------ key splits
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_flash_key_splits(n):
    """L = 700 (22 tiles), Sq = 40: the sequence at position 3 fills two tiles and leaves most splits empty
    (they publish m = -1e30, l = 0), the one at 600 fills every split."""
    B, Hkv, H, D, Sq, Lk = 2, 2, 4, 128, 40, 700
    g = torch.Generator(device="cuda").manual_seed(n)
    kc = torch.randn(B, Lk, Hkv, D, device="cuda", generator=g)
    vc = torch.randn(B, Lk, Hkv, D, device="cuda", generator=g)
    q = torch.randn(B, Sq, H, D, device="cuda", generator=g)
    pos = _pos(3, 600)
    f32 = T.sdpa_cache(q, kc, vc, pos, flash=False)
    T.set_attention_h3g_kvsplit(n)
    try:
        got = T.sdpa_cache(q, kc, vc, pos, flash=True)
    finally:
        T.set_attention_h3g_kvsplit(0)
    _close_to_fp64(got, _ref64(q, kc, vc, pos), f32)


# ------------------------------------------------------------------ ring caches
LIMIT = 200


def _ring_caches(B, C, Hkv, D, pos, Sq, g):
    """Ring caches as they stand after the step's writes: slot s of sequence b holds the row of the position
    pmax - ((pmax - s) mod C) of a long random sequence; slots never written (a negative position; every slot
    of a sequence with a bad counter) hold NaN."""
    seq_k = torch.randn(B, LIMIT, Hkv, D, device="cuda", generator=g)
    seq_v = torch.randn(B, LIMIT, Hkv, D, device="cuda", generator=g)
    kc = torch.full((B, C, Hkv, D), float("nan"), device="cuda")
    vc = torch.full((B, C, Hkv, D), float("nan"), device="cuda")
    for b, p0 in enumerate(pos):
        if not 0 <= p0 < LIMIT:
            continue
        pmax = p0 + Sq - 1
        for s in range(C):
            a = pmax - ((pmax - s) % C)
            if a >= 0:
                kc[b, s], vc[b, s] = seq_k[b, a], seq_v[b, a]
    return kc, vc


@pytest.mark.parametrize("D, H, Hkv", [(128, 4, 2), (64, 8, 1)])
@pytest.mark.parametrize("W, Sq, C, wrapped", [(8, 5, 12, 30), (8, 40, 47, 100), (1, 33, 33, 70), (64, 33, 96, 160)])
@pytest.mark.parametrize("rope", [False, True])
def test_flash_over_ring_caches_matches_fp64(D, H, Hkv, W, Sq, C, wrapped, rope):
    """Four sequences: one whose ring has wrapped at least twice, one at position 2 (most slots never written:
    NaN, not read), one at -1 and one at the limit (zero rows).  W < Sq: the long windowed prefill, every row
    sees its last W keys among the step's own."""
    g = torch.Generator(device="cuda").manual_seed(W + Sq + C + D)
    p = (wrapped, 2, -1, LIMIT)
    assert wrapped + Sq - 1 >= 2 * C and wrapped + Sq <= LIMIT
    kc, vc = _ring_caches(4, C, Hkv, D, p, Sq, g)
    q = torch.randn(4, Sq, H, D, device="cuda", generator=g)
    pos = _pos(*p)
    t64 = _tables64(LIMIT, D) if rope else None
    tabs = tuple(t.float().cuda() for t in t64) if rope else None
    got = T.sdpa_cache(q, kc, vc, pos, rope=tabs, window=W, limit=LIMIT, flash=True)
    f32 = T.sdpa_cache(q, kc, vc, pos, rope=tabs, window=W, limit=LIMIT, flash=False)
    _close_to_fp64(got, _ref64(q, kc, vc, pos, t64, window=W, limit=LIMIT), f32)
    assert float(got[2:].abs().max()) == 0.0


# ------------------------------------------------------------------ refused arguments
def _c_call(D=128, H=4, Hkv=2, Sq=40, Lc=300, window=0, limit=0):
    lib = _lib.lib()
    B = 1
    q = torch.zeros(B, Sq, H, D, device="cuda")
    kc = torch.zeros(B, Lc, Hkv, D, device="cuda")
    pos = _pos(0)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
    wptr = (ws.data_ptr() + 255) // 256 * 256
    out = torch.zeros_like(q)
    args = (q.data_ptr(), H * D, Sq * H * D, kc.data_ptr(), kc.data_ptr(), pos.data_ptr(), None, None, 0,
            out.data_ptr(), H * D, Sq * H * D, B, H, Hkv, Sq, Lc, D, 0.1, wptr, ws.numel() - 256)
    if window:
        return lib.nos_attn_h3g_cache_ring(*args, window, limit, None)
    return lib.nos_attn_h3g_cache(*args, None)


def test_flash_refuses_what_it_does_not_cover():
    assert _c_call(Sq=4, Lc=40) == 0 and _c_call(Sq=4, Lc=12, window=8, limit=64) == 0
    assert _c_call(D=96, Sq=4, Lc=40) == INVALID
    assert _c_call(H=3, Hkv=2, Sq=4, Lc=40) == INVALID
    assert _c_call(Sq=5, Lc=11, window=8, limit=64) == INVALID      # C < min(limit, W + Sq - 1)
    assert _lib.lib().nos_attn_h3g_cache_workspace(1, 4, 2, 4, 40, 96) == -1
    torch.cuda.synchronize()
    q = torch.zeros(1, 4, 4, 128, device="cuda")
    kc = torch.zeros(1, 40, 2, 128, device="cuda")
    with pytest.raises(ValueError):
        T.sdpa_cache(q[..., :96].contiguous(), kc[..., :96].contiguous(), kc[..., :96].contiguous(), _pos(0), flash=True)
    with pytest.raises(ValueError):
        T.sdpa_cache(q[:, :, :3].contiguous(), kc, kc, _pos(0), flash=True)
    with pytest.raises(ValueError):
        T.sdpa_cache(torch.zeros(1, 5, 4, 128, device="cuda"), kc[:, :11].contiguous(), kc[:, :11].contiguous(),
                     _pos(0), window=8, limit=64, flash=True)
    with pytest.raises(ValueError, match="flash"):
        T.sdpa_cache(q, kc.bfloat16(), kc.bfloat16(), _pos(0), flash=True)
    with pytest.raises(ValueError, match="flash"):
        T.sdpa_cache(q[:, :1].contiguous(), kc, kc, _pos(0), partials=True, flash=True)
    with pytest.raises(ValueError, match="flash"):
        T.sdpa_cache(q, kc, kc, _pos(0), sync=torch.zeros(2, dtype=torch.int32, device="cuda"), flash=True)


# ------------------------------------------------------------------ CU budget
@pytest.mark.parametrize("ring", [False, True])
def test_flash_under_a_cu_budget_gives_the_same_values(ring):
    """8 CUs: the persistent grid walks several items per workgroup (32 items x 2 key splits at head_dim 128,
    one workgroup per CU); the split count pinned, the bits are those of the unbudgeted launch."""
    B, Hkv, H, D, Sq = 2, 2, 8, 128, 290
    g = torch.Generator(device="cuda").manual_seed(8)
    kw = dict(window=64, limit=1024) if ring else {}
    Lc = 353 if ring else L
    kc = torch.randn(B, Lc, Hkv, D, device="cuda", generator=g)
    vc = torch.randn(B, Lc, Hkv, D, device="cuda", generator=g)
    q = torch.randn(B, Sq, H, D, device="cuda", generator=g)
    pos = _pos(4, 500) if ring else _pos(4, 10)
    T.set_attention_h3g_kvsplit(2)
    want = T.sdpa_cache(q, kc, vc, pos, flash=True, **kw)
    ops.set_cu_budget(8)
    try:
        got = T.sdpa_cache(q, kc, vc, pos, flash=True, **kw)
        torch.cuda.synchronize()
    finally:
        ops.set_cu_budget(0)
        T.set_attention_h3g_kvsplit(0)
    assert torch.equal(got, want)
    _close_to_fp64(got, _ref64(q, kc, vc, pos, **kw), T.sdpa_cache(q, kc, vc, pos, flash=False, **kw))
