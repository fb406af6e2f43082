"""The decode kernels' bf16, strided and multi-group paths (csrc/hip/decode.hip:
``gemv_kernel``, ``attn_decode_kernel``, ``kv_write_kernel``) and a bf16 decoder
tenant on the GPU.  Two derived criteria, no measured tolerance:

* the fp32 bar: max |got - ref64| / max |ref64| <= max(4 e32, 2e-6), ref64 the
  same operation in fp64 on the same input values, e32 torch fp32's own error
  (decode attention: the absolute form of ``test_decode_attention_matches_fp64``);
* the bf16-of-fp32 identity: the kernels widen bf16 inputs exactly, do the same
  fp32 arithmetic and round the result once to nearest even, so a call with
  bf16 activations equals, bit for bit, the call on ``.float()`` copies passed
  through ``.bfloat16()``.

Inputs are drawn on the CPU from seeded generators; references run on the CPU."""
from __future__ import annotations

import copy
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402
from nos_amd.ops import EPI_BIAS, EPI_RESID, _lib, _stream  # noqa: E402
from nos_amd.ops import tenant as T  # noqa: E402
from nos_amd.podserver.program.reference import kv_write_ref, rotary_at_ref, sdpa_cache_ref  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(autouse=True)
def _h3():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _randn(g: torch.Generator, *shape, dtype=F32) -> torch.Tensor:
    """Seeded normal values, rounded to ``dtype``, on the GPU."""
    return torch.randn(*shape, generator=g).to(dtype).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------ 1. GEMV
_ACT = {"gelu": F.gelu, "relu": torch.relu, "silu": F.silu}


def _gemv_ref(x, w, b, act, r, rms, glu, dt):
    """act(rms(x) W^T + b) + R (GLU: silu(gate + b) * (up + b)) on the CPU in ``dt``."""
    xd = x.detach().cpu().to(dt)
    if rms:
        xd = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + rms)
    y = xd @ w.detach().cpu().to(dt).t()
    if b is not None:
        y = y + b.detach().cpu().to(dt)
    if glu:
        nh = y.shape[1] // 2
        y = F.silu(y[:, :nh]) * y[:, nh:]
    else:
        y = _ACT.get(act, lambda t: t)(y)
    if r is not None:
        y = y + r.detach().cpu().to(dt)
    return y


def _bar(got, x, w, b=None, act=None, r=None, rms=0.0, glu=False, what=None):
    """The fp32 bar; returns the fp64 reference."""
    ref64 = _gemv_ref(x, w, b, act, r, rms, glu, torch.float64)
    ref32 = _gemv_ref(x, w, b, act, r, rms, glu, F32)
    scale = float(ref64.abs().max()) or 1.0
    e = float((got.detach().cpu().double() - ref64).abs().max()) / scale
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    print(f"{what}: e = {e:.3g}, e32 = {e32:.3g}")
    assert got.shape == ref64.shape and e <= max(4 * e32, 2e-6), (what, e, e32)
    return ref64


def _operands(g, M, N, K, wdt, xdt=F32):
    x = _randn(g, M, K, dtype=xdt)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(wdt).cuda()
    b = _randn(g, N, dtype=wdt)
    return x, w, b


def _raw_gemv(x, w, b, r, y, M, N, K, epi=0, ldx=None) -> int:
    return _lib.lib().nos_gemv(x.data_ptr(), int(x.dtype == BF16), x.stride(0) if ldx is None else ldx, w.data_ptr(),
                               int(w.dtype == BF16), w.stride(0), _ptr(b), _ptr(r), r.stride(0) if r is not None else 0,
                               y.data_ptr(), y.stride(0), M, N, K, epi, 0.0, _stream())


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("N, K", [(7, 256), (1000, 1024), (64, 2816)])
@pytest.mark.parametrize("wdt", [F32, BF16])
def test_gemv_bf16_activations_are_the_fp32_gemv_rounded_once(M, N, K, wdt):
    """bf16 x, residual and y (``xbf``): the bf16-of-fp32 identity, and the fp32
    call at the fp32 bar.  8 rows of K = 2816 are 88 KiB of x, over the kernel's
    64 KiB of LDS: there ``gemv_ok`` must say no and the entry point refuse
    without a launch (``ops.linear`` takes such a product elsewhere)."""
    g = _gen(M + N + K)
    x, w, b = _operands(g, M, N, K, wdt, BF16)
    r = _randn(g, M, N, dtype=BF16)
    if M * K * 4 > 65536:
        assert (M, K) == (8, 2816) and not T.gemv_ok(x, w)
        y = torch.full((M, N), 7.0, dtype=BF16, device="cuda")
        assert _raw_gemv(x, w, b, r, y, M, N, K, EPI_BIAS | EPI_RESID) != 0
        torch.cuda.synchronize()
        assert bool((y == 7.0).all())
        return
    assert T.gemv_ok(x, w)
    for act in (None, "silu"):
        for rms in (0.0, 1e-5):
            got = T.gemv(x, w, b, act, r, rms_eps=rms)
            f32 = T.gemv(x.float(), w, b, act, r.float(), rms_eps=rms)
            assert got.dtype == BF16 and f32.dtype == F32
            assert torch.equal(got, f32.bfloat16()), (act, rms)
            _bar(f32, x, w, b, act, r, rms, what=(act, rms))


def test_gemv_glu_with_bf16_activations():
    g = _gen(11)
    x, w, b = _operands(g, 3, 2 * 500, 1024, BF16, BF16)
    for rms in (0.0, 1e-5):
        got = T.gemv(x, w, b, rms_eps=rms, glu=True)
        f32 = T.gemv(x.float(), w, b, rms_eps=rms, glu=True)
        assert got.dtype == BF16 and got.shape == (3, 500) and torch.equal(got, f32.bfloat16())
        _bar(f32, x, w, b, rms=rms, glu=True, what=("glu", rms))


def _budgeted(cus, f):
    ops.set_cu_budget(cus)
    try:
        return f()
    finally:
        ops.set_cu_budget(0)


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("K", [64, 1028])
@pytest.mark.parametrize("wdt", [F32, BF16])
def test_gemv_walks_several_groups_under_a_cu_budget(M, K, wdt):
    """8 CUs: 128 workgroups over N = 2060's 258 column groups -- two trips each,
    a third for two of them, 4 valid columns in the last group; the prefetched
    first chunk belongs to the first trip only.  No output's summation order
    depends on the grid: equal to the unbudgeted call bit for bit."""
    N = 2060
    g = _gen(M + K)
    x, w, b = _operands(g, M, N, K, wdt)
    r = _randn(g, M, N)
    for rms in (0.0, 1e-5):
        free = T.gemv(x, w, b, "gelu", r, rms_eps=rms)
        got = _budgeted(8, lambda: T.gemv(x, w, b, "gelu", r, rms_eps=rms))
        _bar(got, x, w, b, "gelu", r, rms, what=("budget", rms))
        assert torch.equal(got, free)


@pytest.mark.parametrize("K", [64, 1028])
@pytest.mark.parametrize("wdt", [F32, BF16])
def test_gemv_glu_walks_several_groups_under_a_cu_budget(K, wdt):
    """Nh = 1030: 258 groups of 4 gate / up pairs over 128 workgroups."""
    M, Nh = 3, 1030
    g = _gen(K)
    x, w, b = _operands(g, M, 2 * Nh, K, wdt)
    for rms in (0.0, 1e-5):
        free = T.gemv(x, w, b, rms_eps=rms, glu=True)
        got = _budgeted(8, lambda: T.gemv(x, w, b, rms_eps=rms, glu=True))
        _bar(got, x, w, b, rms=rms, glu=True, what=("glu budget", rms))
        assert got.shape == (M, Nh) and torch.equal(got, free)


@pytest.mark.parametrize("M", [1, 3])
def test_gemv_vocabulary_head_of_128256_rows(M):
    """No budget: 16032 column groups over at most 16 workgroups per CU -- every
    workgroup walks several.  Greedy decoding reads the argmax: equal to fp64's on
    every row whose top two fp64 logits are further apart than 1e-4 of max |y|
    -- and the seed makes that every row."""
    N, K = 128256, 64
    g = _gen(5)
    x = _randn(g, M, K)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).cuda()
    for rms in (0.0, 1e-5):
        got = T.gemv(x, w, rms_eps=rms)
        ref64 = _bar(got, x, w, rms=rms, what=("vocab", rms))
        top = ref64.topk(2, dim=-1).values
        clear = (top[:, 0] - top[:, 1]) > 1e-4 * float(ref64.abs().max())
        assert bool(clear.all()), top
        assert torch.equal(got.argmax(-1).cpu(), ref64.argmax(-1))
        assert torch.equal(T.argmax(got).long().cpu(), ref64.argmax(-1))


@pytest.mark.parametrize("M, K", [(1, 1028), (3, 1028), (1, 3072), (1, 3076), (4, 4096), (1, 11008), (1, 16384)])
@pytest.mark.parametrize("wdt", [F32, BF16])
def test_gemv_k_batches(M, K, wdt):
    """The KU = 12 form: a nearly empty batch (1028), exactly one (3072), a
    one-lane second (3076), four (a 7B-class down projection's 11008) and the
    LDS limit (16384 at M = 1, 4096 at M = 4: 65536 bytes of x)."""
    N = 40
    g = _gen(M + K)
    x, w, b = _operands(g, M, N, K, wdt)
    r = _randn(g, M, N)
    assert T.gemv_ok(x, w)
    for rms in (0.0, 1e-5):
        _bar(T.gemv(x, w, b, None, r, rms_eps=rms), x, w, b, None, r, rms, what=(M, K, rms))


@pytest.mark.parametrize("M", [4, 6, 7])
@pytest.mark.parametrize("wdt", [F32, BF16])
def test_gemv_row_counts_four_six_seven(M, wdt):
    """Each M is its own template instance (the finishing lane is c x M + m)."""
    g = _gen(M)
    x, w, b = _operands(g, M, 9, 256, wdt)
    r = _randn(g, M, 9)
    xg, wg, bg = _operands(g, M, 26, 256, wdt)
    for rms in (0.0, 1e-5):
        _bar(T.gemv(x, w, b, "silu", r, rms_eps=rms), x, w, b, "silu", r, rms, what=(M, rms))
        got = T.gemv(xg, wg, bg, rms_eps=rms, glu=True)
        assert got.shape == (M, 13)
        _bar(got, xg, wg, bg, rms=rms, glu=True, what=(M, "glu", rms))


@pytest.mark.parametrize("Nh", [13, 1030])
@pytest.mark.parametrize("K", [64, 1024])
@pytest.mark.parametrize("wdt", [F32, BF16])
def test_gemv_glu_tails_and_bias(Nh, K, wdt):
    """Nh % 4 != 0 (the ``n0 < Nh`` tail: one or two waves of the last group
    finish nothing), a bias of 2 Nh entries (gate's and up's halves), bf16 W."""
    for M in (2, 8):
        g = _gen(Nh + K + M)
        x, w, b = _operands(g, M, 2 * Nh, K, wdt)
        for bias in (None, b):
            for rms in (0.0, 1e-5):
                got = T.gemv(x, w, bias, rms_eps=rms, glu=True)
                assert got.shape == (M, Nh)
                _bar(got, x, w, bias, rms=rms, glu=True, what=(M, bias is not None, rms))


@pytest.mark.parametrize("xdt", [F32, BF16])
@pytest.mark.parametrize("wdt", [F32, BF16])
def test_gemv_strided_operands(xdt, wdt):
    """x a column slice, W a row slice of a wider matrix, the residual and
    ``out=`` column slices: the strides reach the kernel (``ldx``, ``ldw``,
    ``ldr``, ``ldy``), nothing outside the slices is read (NaN there) or written."""
    nan = float("nan")
    g = _gen(3)
    xs = torch.full((3, 512), nan, dtype=xdt, device="cuda")
    xs[:, 128:384] = _randn(g, 3, 256, dtype=xdt)
    ws = torch.full((40, 512), nan, dtype=wdt, device="cuda")
    ws[:, :256] = _randn(g, 40, 256, dtype=wdt) / 16
    rs = torch.full((3, 128), nan, dtype=xdt, device="cuda")
    rs[:, 24:64] = _randn(g, 3, 40, dtype=xdt)
    b = _randn(g, 40, dtype=wdt)
    x, w, r = xs[:, 128:384], ws[:, :256], rs[:, 24:64]
    assert T.gemv_ok(x, w) and not x.is_contiguous() and not w.is_contiguous() and not r.is_contiguous()
    for rms in (0.0, 1e-5):
        buf = torch.full((3, 64), nan, dtype=xdt, device="cuda")
        out = buf[:, 8:48]
        got = T.gemv(x, w, b, "silu", r, out=out, rms_eps=rms)
        want = T.gemv(x.contiguous(), w.contiguous(), b, "silu", r.contiguous(), rms_eps=rms)
        assert got is out and bool(torch.isfinite(want.float()).all()) and torch.equal(out, want)
        assert bool(torch.isnan(buf[:, :8]).all()) and bool(torch.isnan(buf[:, 48:]).all())
        if xdt == F32:
            _bar(want, x, w, b, "silu", r, rms, what=("strided", rms))


@pytest.mark.parametrize("case", ["k-not-4", "nine-rows", "x-over-lds", "ldx-below-k", "misaligned-w", "glu-odd-n",
                                  "glu-residual", "bias-null"])
def test_gemv_refuses_bad_arguments_without_a_launch(case):
    M, N, K, epi, ldx = 2, 8, 64, 0, None
    if case == "k-not-4":
        K = 62
    elif case == "nine-rows":
        M = 9
    elif case == "x-over-lds":
        M, K = 1, 16388            # M x K x 4 = 65536 + 16
    elif case == "ldx-below-k":
        ldx = K - 4
    elif case == "glu-odd-n":
        N, epi = 7, T.EPI_GLU
    elif case == "glu-residual":
        epi = T.EPI_GLU | EPI_RESID
    elif case == "bias-null":
        epi = EPI_BIAS
    Ka = max(K, 64)
    x = torch.ones(M, Ka, device="cuda")
    store = torch.ones(N * Ka + 4, device="cuda")
    off = 2 if case == "misaligned-w" else 0           # 8 bytes off 16-byte alignment
    w = store[off:off + N * Ka].view(N, Ka)
    assert (w.data_ptr() % 16 == 8) == (case == "misaligned-w")
    r = torch.ones(M, N, device="cuda") if case == "glu-residual" else None
    y = torch.full((M, N), 7.0, device="cuda")
    assert _raw_gemv(x, w, None, r, y, M, N, K, epi, ldx) != 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    # gemv_ok speaks of the product's shape, strides and alignment, not of the epilogue or a forged ldx
    assert T.gemv_ok(x[:, :K], w[:, :K]) == (case in ("ldx-below-k", "glu-odd-n", "glu-residual", "bias-null"))


# ------------------------------------------------------------------ 2. decode attention
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


def _attn_bar(got, q, kc, vc, pos, tabs=None, what=None):
    """``test_decode_attention_matches_fp64``'s bar: e <= max(4 e32, 2e-6) against fp64."""
    p = pos.cpu()
    ref64 = sdpa_cache_ref(_rot64(q, tabs, p), kc.double().cpu(), vc.double().cpu(), p)
    q32 = q.float().cpu()
    if tabs is not None:
        q32 = rotary_at_ref(q32, tabs[0].cpu(), tabs[1].cpu(), p)
    ref32 = sdpa_cache_ref(q32, kc.float().cpu(), vc.float().cpu(), p)
    e = float((got.double().cpu() - ref64).abs().max())
    e32 = float((ref32.double() - ref64).abs().max())
    print(f"{what}: e = {e:.3g}, e32 = {e32:.3g}")
    assert got.shape == ref64.shape and e <= max(4 * e32, 2e-6), (what, e, e32)


def _pos(*v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _synced(q, kc, vc, pos, n, **kw):
    """The same call with the combine folded into the decode launch; the counters end zero."""
    sync = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = T.sdpa_cache(q, kc, vc, pos, sync=sync, **kw)
    assert int(sync.abs().sum()) == 0
    return out


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G, Sq", [(4, 1), (8, 5)])
@pytest.mark.parametrize("cdt", [F32, BF16])
def test_decode_attention_bf16_q_is_the_fp32_call_rounded_once(D, G, Sq, cdt):
    B, Hkv, L = 2, 2, 300
    H = G * Hkv
    g = _gen(D + G + Sq)
    kc, vc = _randn(g, B, L, Hkv, D, dtype=cdt), _randn(g, B, L, Hkv, D, dtype=cdt)
    q = _randn(g, B, Sq, H, D, dtype=BF16)
    pos = _pos(0, max(0, L - Sq - 3))
    for tabs in (None, _tables(L, D)):
        f32 = T.sdpa_cache(q.float(), kc, vc, pos, rope=tabs)
        got = T.sdpa_cache(q, kc, vc, pos, rope=tabs)
        assert got.dtype == BF16 and torch.equal(got, f32.bfloat16())
        _attn_bar(f32, q, kc, vc, pos, tabs, what=("bf16 q", tabs is not None))
        assert torch.equal(_synced(q, kc, vc, pos, B * Hkv, rope=tabs), got)


@pytest.mark.parametrize("Sq", [1, 9])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_decode_attention_takes_q_as_a_slice_of_a_fused_projection(Sq, dt):
    """q = the first H x D columns of a [B, Sq, (H + 2 Hkv) x D] projection
    (``ldq``, ``bsq``), also with the step's K / V rows (``fresh=``) from the
    same projection's other columns."""
    B, Hkv, G, D, L = 2, 2, 4, 128, 300
    H = G * Hkv
    g = _gen(Sq)
    kc, vc = _randn(g, B, L, Hkv, D, dtype=dt), _randn(g, B, L, Hkv, D, dtype=dt)
    proj = torch.full((B, Sq, (H + 2 * Hkv) * D), float("nan"), dtype=dt, device="cuda")
    proj[..., :H * D] = _randn(g, B, Sq, H * D, dtype=dt)
    q = proj[..., :H * D].view(B, Sq, H, D)
    pos = _pos(5, 126)
    assert not q.is_contiguous()
    got = T.sdpa_cache(q, kc, vc, pos)
    assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, T.sdpa_cache(q.contiguous(), kc, vc, pos))
    proj[..., H * D:] = _randn(g, B, Sq, 2 * Hkv * D, dtype=dt)
    kx = proj[..., H * D:(H + Hkv) * D].view(B, Sq, Hkv, D)
    vx = proj[..., (H + Hkv) * D:].view(B, Sq, Hkv, D)
    tabs = _tables(L, D)
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    got = T.sdpa_cache(q, k1, v1, pos, rope=tabs, fresh=(kx, vx))
    want = T.sdpa_cache(q.contiguous(), k2, v2, pos, rope=tabs, fresh=(kx.contiguous(), vx.contiguous()))
    assert torch.equal(got, want) and torch.equal(k1, k2) and torch.equal(v1, v2)
    assert not torch.equal(k1, kc) and not torch.equal(v1, vc)


def _workspace_bytes(B, Hkv, G, Sq, L, D):
    return B * Hkv * -(-L // 128) * G * min(Sq, max(32 // G, 1)) * (D + 2) * 4


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G, Sq", [(3, 1), (3, 11), (5, 7), (32, 1), (32, 2)])
@pytest.mark.parametrize("L", [16, 300])
def test_decode_attention_group_sizes_that_do_not_divide_32(D, G, Sq, L):
    """32 // G query tokens per launch: G = 3 -> 10 (30 rows; Sq = 11 is two
    launches of 10 + 1), G = 5 -> 6 (Sq = 7: 6 + 1), G = 32 -> one token per launch."""
    assert Sq <= L
    B, Hkv = 2, 1 if G == 32 else 2
    H = G * Hkv
    g = _gen(D + G + Sq + L)
    q = _randn(g, B, Sq, H, D)
    pos = _pos(0, max(0, L - Sq - 3))
    assert int(_lib.lib().nos_attn_decode_workspace(B, H, Hkv, Sq, L, D)) == _workspace_bytes(B, Hkv, G, Sq, L, D)
    for cdt in (F32, BF16):
        kc, vc = _randn(g, B, L, Hkv, D, dtype=cdt), _randn(g, B, L, Hkv, D, dtype=cdt)
        got = T.sdpa_cache(q, kc, vc, pos)
        _attn_bar(got, q, kc, vc, pos, what=(G, Sq, cdt))
        assert torch.equal(_synced(q, kc, vc, pos, B * Hkv), got)


def test_decode_attention_refuses_33_query_heads_per_kv_head():
    B, Sq, Hkv, G, D, L = 1, 1, 1, 33, 64, 16
    q = torch.ones(B, Sq, G, D, device="cuda")
    kc, vc = torch.ones(B, L, Hkv, D, device="cuda"), torch.ones(B, L, Hkv, D, device="cuda")
    pos = _pos(3)
    with pytest.raises(RuntimeError, match="nos_attn_decode"):
        T.sdpa_cache(q, kc, vc, pos)
    out = torch.full((B, Sq, G, D), 7.0, device="cuda")
    ws = torch.zeros(1 << 16, device="cuda")
    rc = _lib.lib().nos_attn_decode(q.data_ptr(), 0, G * D, Sq * G * D, kc.data_ptr(), vc.data_ptr(), 0, pos.data_ptr(),
                                    None, None, 0, out.data_ptr(), 0, B, G, Hkv, Sq, L, D, 1.0 / math.sqrt(D),
                                    ws.data_ptr(), ws.numel() * 4, None, None, 0, 0, 0, 0, 0, 0, None, 0, 0, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == 7.0).all())


@pytest.mark.parametrize("cdt", [F32, BF16])
@pytest.mark.parametrize("fdt", [F32, BF16])
@pytest.mark.parametrize("rope", [False, True])
def test_decode_attention_attends_the_fresh_rows_as_the_cache_holds_them(cdt, fdt, rope):
    """``fresh=`` on every cache / row dtype pair: the caches and the output of
    ``kv_write`` + ``sdpa_cache`` -- the step attends its own K / V rows at the
    cache's precision (a bf16 cache holds them rounded), as the later query
    launches of the same call and the next step do."""
    B, L, Hkv, G, D = 2, 300, 2, 4, 128
    H = G * Hkv
    tabs = _tables(L, D) if rope else None
    pos = _pos(5, 126)                                   # the second crosses a 128-key split
    for Sq in (1, 3, 20):
        g = _gen(Sq + G)
        kc, vc = _randn(g, B, L, Hkv, D, dtype=cdt), _randn(g, B, L, Hkv, D, dtype=cdt)
        q = _randn(g, B, Sq, H, D)
        kx = _randn(g, B, Sq, 3 * Hkv, D, dtype=fdt)[:, :, :Hkv]     # strided rows, as from a fused projection
        vx = _randn(g, B, Sq, Hkv, D, dtype=fdt)
        kc2, vc2 = kc.clone(), vc.clone()
        T.kv_write(kc2, kx, pos, rope=tabs, second=(vc2, vx))
        ref = T.sdpa_cache(q, kc2, vc2, pos, rope=tabs)
        got = T.sdpa_cache(q, kc, vc, pos, rope=tabs, fresh=(kx, vx))
        torch.cuda.synchronize()
        assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
        print(f"Sq = {Sq}: max |fresh - written| = {float((got - ref).abs().max()):.3g}")
        torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-6)


def test_decode_attention_of_one_fresh_key_returns_the_cached_value():
    """Position 0, one query token: the only visible key is the fresh one, so
    the output IS the V row -- the bf16 value the cache now holds, bit for bit,
    not the fp32 row it was rounded from."""
    B, L, Hkv, G, D = 2, 300, 2, 4, 128
    g = _gen(0)
    kc, vc = _randn(g, B, L, Hkv, D, dtype=BF16), _randn(g, B, L, Hkv, D, dtype=BF16)
    q = _randn(g, B, 1, G * Hkv, D)
    kx, vx = _randn(g, B, 1, Hkv, D), _randn(g, B, 1, Hkv, D)
    assert bool((vx.bfloat16().float() != vx).float().mean() > 0.9)      # not bf16-representable
    got = T.sdpa_cache(q, kc, vc, _pos(0, 0), fresh=(kx, vx))
    assert torch.equal(vc[:, 0], vx[:, 0].bfloat16()) and torch.equal(kc[:, 0], kx[:, 0].bfloat16())
    want = vc[:, 0].float().repeat_interleave(G, dim=1)                  # [B, H, D]
    print(f"max |out - cached V| / max |V| = {float((got[:, 0] - want).abs().max() / want.abs().max()):.3g}")
    assert torch.equal(got[:, 0], want)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq", [1, 5])
@pytest.mark.parametrize("cdt", [F32, BF16])
@pytest.mark.parametrize("fill", [float("nan"), float("inf")])
def test_decode_attention_never_reads_rows_past_the_visible_keys(D, Sq, cdt, fill):
    """Cache rows >= pos[b] + Sq are unwritten memory: NaN or +inf there must not
    reach the output (not even as 0 x V) -- the same bits as with zeros there."""
    B, L, Hkv, G = 3, 300, 2, 4
    H = G * Hkv
    g = _gen(D + Sq)
    kc, vc = _randn(g, B, L, Hkv, D, dtype=cdt), _randn(g, B, L, Hkv, D, dtype=cdt)
    q = _randn(g, B, Sq, H, D)
    pos = _pos(0, 120, 250)
    kz, vz, kb, vb = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    for b, p in enumerate(pos.tolist()):
        kz[b, p + Sq:] = 0
        vz[b, p + Sq:] = 0
        kb[b, p + Sq:] = fill
        vb[b, p + Sq:] = fill
    want = T.sdpa_cache(q, kz, vz, pos)
    got = T.sdpa_cache(q, kb, vb, pos)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    _attn_bar(got, q, kz, vz, pos, what=(D, Sq, cdt))
    assert torch.equal(_synced(q, kb, vb, pos, B * Hkv), want)
    if Sq == 1:
        w = _randn(g, 48, H * D) / 16
        y = T.gemv_partials(T.sdpa_cache(q, kb, vb, pos, partials=True), w)
        assert bool(torch.isfinite(y).all())
        assert torch.equal(y, T.gemv_partials(T.sdpa_cache(q, kz, vz, pos, partials=True), w))
        assert torch.equal(y, T.gemv(want.reshape(B, H * D), w))


@pytest.mark.parametrize("Sq", [1, 5])
@pytest.mark.parametrize("outliers", [False, True])
def test_decode_attention_with_large_logits(Sq, outliers):
    """Logits of +-100 (q x 30), and one key of the first split at 8 x, one of the
    last at -8 x: a split's whole partial underflows against another's in the
    log-sum-exp combine -- finite, at the fp64 bar, the same bits in all three
    combine forms."""
    B, L, Hkv, G, D = 2, 1100, 2, 4, 128
    H = G * Hkv
    g = _gen(Sq + 2 * outliers)
    kc, vc = _randn(g, B, L, Hkv, D), _randn(g, B, L, Hkv, D)
    q = _randn(g, B, Sq, H, D) * 30
    if outliers:
        kc[:, 5] *= 8
        kc[:, 1050] *= -8
    pos = _pos(L - Sq - 3, L - Sq)
    got = T.sdpa_cache(q, kc, vc, pos)
    assert bool(torch.isfinite(got).all())
    _attn_bar(got, q, kc, vc, pos, what=("large", Sq, outliers))
    assert torch.equal(_synced(q, kc, vc, pos, B * Hkv), got)
    if Sq == 1:
        w = _randn(g, 48, H * D) / 16
        y = T.gemv_partials(T.sdpa_cache(q, kc, vc, pos, partials=True), w)
        assert bool(torch.isfinite(y).all()) and torch.equal(y, T.gemv(got.reshape(B, H * D), w))


# ------------------------------------------------------------------ 3. kv_write across dtypes
@pytest.mark.parametrize("xdt, cdt", [(F32, BF16), (BF16, F32)])
@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("second", [False, True])
def test_kv_write_converts_between_the_row_and_the_cache_dtype(xdt, cdt, rope, second):
    """``xbf`` != ``cbf``: a conversion only (exact), or the rotation of the
    rows' values in fp32 stored in the cache's dtype -- the kernel rounds once,
    into the cache, never to the rows' dtype on the way."""
    B, L, H, D, S = 3, 40, 2, 64, 5
    g = _gen(7)
    cache, cache2 = _randn(g, B, L, H, D, dtype=cdt), _randn(g, B, L, H, D, dtype=cdt)
    x = _randn(g, B, S, 3 * H * D, dtype=xdt)[..., H * D:2 * H * D].view(B, S, H, D)     # strided rows
    x2 = _randn(g, B, S, H, D, dtype=xdt)
    pos = _pos(0, 17, L - 2)                                                              # the last overflows
    tabs = _tables(L, D) if rope else None
    xr = rotary_at_ref(x.float().cpu(), tabs[0].cpu(), tabs[1].cpu(), pos.cpu()) if rope else x.cpu()
    ref = kv_write_ref(cache.clone().cpu(), xr, pos.cpu())
    ref2 = kv_write_ref(cache2.clone().cpu(), x2.cpu(), pos.cpu())
    before2 = cache2.clone()
    got = T.kv_write(cache, x, pos, rope=tabs, second=(cache2, x2) if second else None)
    assert got is cache and got.dtype == cdt and ref.dtype == cdt
    if rope:
        tol = 1e-6 if cdt == F32 else 1e-2
        torch.testing.assert_close(got.cpu().float(), ref.float(), rtol=tol, atol=tol)
    else:
        assert torch.equal(got.cpu(), ref)
    assert torch.equal(cache2.cpu(), ref2) if second else torch.equal(cache2, before2)    # V: never rotated


# ------------------------------------------------------------------ 4. a bf16 decoder tenant
def test_bf16_decoder_tenant_on_the_gpu():
    """The tiny Llama as a bf16 tenant (bf16 activations and caches): prefill +
    3 decode steps compiled for the GPU.  The step program keeps the fp32
    program's fusions except the fp32-only fold of the split combine into the
    O-projection.  The last step's logits against ref64, the model in fp64 on
    its bf16-rounded weights, relative to max |ref64|: the GPU's error at most
    twice that of the same programs compiled for the CPU (both round the
    activations to bf16 at the same graph edges; two for the summation orders).
    Measured on an MI355X: e_gpu = 4.56e-3, e_cpu = 4.32e-3."""
    from nos_amd.models.llama_program import llama_config, llama_decode_programs, llama_model
    from nos_amd.podserver import program as PG

    m = llama_model(llama_config(False), 0)
    progs, w = llama_decode_programs(m, 8, 64, dtype="bf16")
    ps = PG.parse_variants(progs, w, gpu=True)
    params, state = ps[0].tensors("cuda"), ps[0].state_tensors("cuda")
    assert state["kc0"].dtype == BF16 and params["lm_head.weight"].dtype == BF16
    pre, step = (p.compile("cuda", params=params, state=state) for p in ps)
    progs32, w32 = llama_decode_programs(m, 8, 64)
    ps32 = PG.parse_variants(progs32, w32, gpu=True)
    step32 = ps32[1].compile("cuda", params=ps32[0].tensors("cuda"))
    for key in ("kv_writes_into_attention", "kv_writes_paired", "rotary_at_fused", "gemv_glu_fused"):
        assert step.stats[key] > 0 and step.stats[key] == step32.stats[key], (key, step.stats, step32.stats)
    assert step32.stats["decode_combines_into_gemv"] == 2 and step.stats["decode_combines_into_gemv"] == 0

    prompt = torch.randint(0, m.config.vocab_size, (1, 8), generator=_gen(0))
    toks = []
    with torch.no_grad():
        logits, nxt = pre(prompt.int().cuda())
        for _ in range(3):
            toks.append(nxt.view(1, 1).int())
            logits, nxt = step(toks[-1])
    assert logits.dtype == BF16 and state["pos"].tolist() == [11]
    seq = torch.cat([prompt] + [t.cpu().long() for t in toks], 1)

    # the same programs on the CPU (the eager reference ops), fed the same tokens
    cs = PG.parse_variants(progs, w)
    cparams, cstate = cs[0].tensors("cpu"), cs[0].state_tensors("cpu")
    cpre, cstep = (p.compile("cpu", params=cparams, state=cstate) for p in cs)
    with torch.no_grad():
        clogits = cpre(prompt.int())[0]
        for t in toks:
            clogits = cstep(t.cpu())[0]
        m64 = copy.deepcopy(m)
        for p in m64.parameters():
            p.copy_(p.bfloat16().float())
        ref64 = m64.double()(seq).logits[:, -1:]
    assert cstate["pos"].tolist() == [11] and clogits.shape == ref64.shape == logits.shape
    scale = float(ref64.abs().max())
    e_gpu = float((logits.double().cpu() - ref64).abs().max()) / scale
    e_cpu = float((clogits.double() - ref64).abs().max()) / scale
    print(f"bf16 tenant: e_gpu = {e_gpu:.3g}, e_cpu = {e_cpu:.3g}")
    assert e_gpu <= 2 * e_cpu, (e_gpu, e_cpu)
