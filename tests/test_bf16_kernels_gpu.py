"""The bf16 pod kernels -- ``nos_gemm_bf16`` / ``nos_gemm_ln_bf16`` (gemm.hip),
``nos_attn_fwd_d64`` (attention.hip), ``nos_layernorm_bf16`` (layernorm.hip)
-- element by element against fp64 references.

Inputs are drawn on the CPU from a seeded generator and rounded to bf16; the
references are computed in fp64 FROM THOSE bf16 VALUES, so the only errors
left are the kernel's own: fp32 accumulation and ONE rounding of the fp32
result to bf16 (unit roundoff u = 2^-8).  Every bound is per element and
derived, not fitted (docs/kernels.md lists the measured error / bound ratios):

* GEMM:       u |ref| + K 2^-23 1.13 den + g,  den = |x| |w|^T + |b|;
              1.13 is GELU's Lipschitz constant (used for every activation),
              g = 1e-6 |pre| with GELU (the kernel's erf is the A&S 7.1.26
              polynomial, 1.5e-7 absolute, on hardware rcp / exp2), else 0;
* LN-fused:   the same with den = rstd (|x| |wg|^T + |mu| rowsum|wg|) + |c2|;
* attention:  (2^-7 + 2^-11) P |v|: one u for P rounded to bf16 before P.V,
              one u for the output, u / 16 for the fp32 scores and exponents;
* LayerNorm:  u |ref| + D 2^-23 ((|s| + |mean|) rstd |gamma| + |beta|), and
              the written sum bit for bit.

Strided cases put NaN between the input rows and a sentinel between the output
rows; a persistent grid must reproduce the one-workgroup-per-tile output bit
for bit.  Each test prints its worst error / bound ratio (``RATIO ...``)."""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from nos_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -8      # bf16 unit roundoff
F32 = 2.0 ** -23   # fp32 accumulation term, per addend
LIP = 1.13         # Lipschitz constant of GELU
SENT = -768.0      # exact in bf16
PAD = 64           # elements of padding before and after a strided buffer (128 bytes: keeps the alignment)
NAN = math.nan

POLICIES = ("throughput", "narrow", "big", "wide")  # 128x128 at these sizes (test_gemm_tile_choice.py), 128x64, 256x256, 256x192
KS = (64, 128, 192, 320)                             # one, two, three and five stages through the 2-deep ring
GEMM_SHAPES = ((300, 264), (300, 260), (9, 4), (9, 8), (33, 7))
# (bias, act, residual)
EPILOGUES = ((False, None, False), (True, None, False), (True, "gelu", False), (True, "relu", False),
             (True, None, True), (True, "gelu", True), (False, "relu", True))


@pytest.fixture(autouse=True)
def _native():
    from nos_amd.ops import _lib

    _lib.require_native_on_gpu()


def _randn(g: torch.Generator, *shape, scale: float = 1.0, shift: float = 0.0) -> torch.Tensor:
    return (torch.randn(*shape, generator=g) * scale + shift).bfloat16()


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def _worst(y: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, rows=None) -> float:
    """max error / bound of y (bf16, any device) against ref (fp64, CPU)."""
    y = y.detach().cpu().double()
    assert y.shape == ref.shape
    if rows is not None:
        y, ref, bound = y[rows], ref[rows], bound[rows]
    assert torch.isfinite(y).all()
    return ((y - ref).abs() / bound.clamp_min(1e-300)).max().item()


def _act64(pre: torch.Tensor, act: str | None) -> torch.Tensor:
    return F.gelu(pre) if act == "gelu" else pre.clamp_min(0) if act == "relu" else pre


def _gemm_bound(pre: torch.Tensor, den: torch.Tensor, act: str | None, r, K: int):
    ref = _act64(pre, act)
    if r is not None:
        ref = ref + r
    g = 1e-6 * pre.abs() if act == "gelu" else 0.0
    return ref, U * ref.abs() + K * F32 * LIP * den + g


# ------------------------------------------------------------------ A. GEMM
@functools.lru_cache(maxsize=None)
def _gemm_data(M: int, N: int, K: int) -> SimpleNamespace:
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    x, w, b, r = _randn(g, M, K, scale=3.0), _randn(g, N, K, scale=0.1), _randn(g, N), _randn(g, M, N)
    xd, wd = x.double(), w.double()
    return SimpleNamespace(x=x, w=w, b=b, r=r, pre=xd @ wd.t(), den=xd.abs() @ wd.abs().t(),
                           dx=x.to(DEV), dw=w.to(DEV), db=b.to(DEV), dr=r.to(DEV))


def _plain_ref(d: SimpleNamespace, bias: bool, act, resid: bool, K: int):
    pre = d.pre + d.b.double() if bias else d.pre
    den = d.den + d.b.double().abs() if bias else d.den
    return _gemm_bound(pre, den, act, d.r.double() if resid else None, K)


@pytest.mark.parametrize("M,N", GEMM_SHAPES)
@pytest.mark.parametrize("policy", POLICIES)
def test_gemm_tiles_k_and_epilogues(policy, M, N):
    """Every tile x K x epilogue.  (300, 264) gives every tile at least 2 x 2
    tiles with a tail each way; N = 260 makes ldc and ldr no multiple of 8 (the
    scalar store path, with and without a residual); (9, 8) is the vector path
    at its smallest N, (9, 4) and (33, 7) are N < 8."""
    worst, where = 0.0, None
    ops.set_gemm_policy(policy)
    try:
        outs = []
        for K in KS:
            d = _gemm_data(M, N, K)
            for bias, act, resid in EPILOGUES:
                y = ops.linear(d.dx, d.dw, d.db if bias else None, act=act, residual=d.dr if resid else None)
                assert y.shape == (M, N) and y.dtype == torch.bfloat16
                outs.append((K, bias, act, resid, y))
    finally:
        ops.set_gemm_policy("throughput")
    for K, bias, act, resid, y in outs:
        ref, bound = _plain_ref(_gemm_data(M, N, K), bias, act, resid, K)
        ratio = _worst(y, ref, bound)
        if ratio > worst:
            worst, where = ratio, (K, bias, act, resid)
    print(f"RATIO gemm_plain {policy} {M}x{N}: {worst:.3f} at (K, bias, act, residual) = {where}")
    assert worst <= 1.0, (worst, where)


def _kind_rows(g: torch.Generator, rows: int, D: int, const_row: int, period: int = 3) -> torch.Tensor:
    """Rows of four kinds: mean 0.5 / std 2, mean 100 / std 1, mean 0 / std 1e-3 (cycling), one constant row."""
    x = torch.empty(rows, D)
    for i in range(rows):
        scale, shift = ((2.0, 0.5), (1.0, 100.0), (1e-3, 0.0))[i % period % 3]
        x[i] = torch.randn(D, generator=g) * scale + shift
    if 0 <= const_row < rows:
        x[const_row] = 1.5
    return x.bfloat16()


@functools.lru_cache(maxsize=None)
def _ln_gemm_data(M: int, N: int, K: int) -> SimpleNamespace:
    g = torch.Generator().manual_seed(7 + 1000003 * M + 1009 * N + K)
    const = M // 2
    x = _kind_rows(g, M, K, const)
    w, b, gamma, beta = _randn(g, N, K, scale=0.1), _randn(g, N), _randn(g, K), _randn(g, K)
    wg, c1, c2 = ops.fold_layernorm(w, b, gamma, beta)  # on the CPU: wg bf16, c1 / c2 fp32
    xd, wgd = x.double(), wg.double()
    mu, var = xd.mean(-1, keepdim=True), xd.var(-1, unbiased=False, keepdim=True)
    return SimpleNamespace(x=x, wg=wg, c1=c1, c2=c2, const=const, xd=xd, wgd=wgd, mu=mu, var=var,
                           xw_abs=xd.abs() @ wgd.abs().t(), wsum=wgd.abs().sum(-1)[None, :],
                           dx=x.to(DEV), dwg=wg.to(DEV), dc1=c1.to(DEV), dc2=c2.to(DEV))


def _ln_ref(d: SimpleNamespace, act, eps: float, K: int):
    rstd = 1.0 / torch.sqrt(d.var + eps)
    c2 = d.c2.double()[None, :]
    pre = ((d.xd - d.mu) * rstd) @ d.wgd.t() + c2
    den = rstd * (d.xw_abs + d.mu.abs() * d.wsum) + c2.abs()
    return _gemm_bound(pre, den, act, None, K)


@pytest.mark.parametrize("M,N", GEMM_SHAPES)
@pytest.mark.parametrize("policy", POLICIES)
def test_gemm_ln_fused(policy, M, N):
    """LayerNorm folded into the GEMM, rows of four kinds in one matrix.  At
    eps = 1e-12 the constant row (variance 0, rstd = 1e6) only has to come out
    finite; its bound is checked at eps = 1e-5, where rstd is well conditioned."""
    worst, where = 0.0, None
    ops.set_gemm_policy(policy)
    try:
        outs = []
        for K in KS:
            d = _ln_gemm_data(M, N, K)
            for act in (None, "gelu", "relu"):
                for eps in (1e-12, 1e-5):
                    outs.append((K, act, eps, ops.linear_ln(d.dx, d.dwg, d.dc1, d.dc2, act=act, eps=eps)))
    finally:
        ops.set_gemm_policy("throughput")
    for K, act, eps, y in outs:
        d = _ln_gemm_data(M, N, K)
        ref, bound = _ln_ref(d, act, eps, K)
        assert torch.isfinite(y.float()).all()
        rows = None if eps > 1e-8 else torch.arange(M) != d.const
        ratio = _worst(y, ref, bound, rows)
        if ratio > worst:
            worst, where = ratio, (K, act, eps)
    print(f"RATIO gemm_ln {policy} {M}x{N}: {worst:.3f} at (K, act, eps) = {where}")
    assert worst <= 1.0, (worst, where)


def _place(src: torch.Tensor, ld: int, fill: float) -> tuple[torch.Tensor, torch.Tensor]:
    """src [rows, cols] on the device at row stride ld, `fill` between the rows
    and in PAD elements before and after; returns (buffer, view)."""
    rows, cols = src.shape
    buf = torch.full((2 * PAD + (rows - 1) * ld + cols,), fill, dtype=src.dtype, device=DEV)
    view = buf.as_strided((rows, cols), (ld, 1), PAD)
    view.copy_(src)
    return buf, view


def _out(rows: int, cols: int, ld: int) -> tuple[torch.Tensor, torch.Tensor]:
    return _place(torch.full((rows, cols), SENT, dtype=torch.bfloat16), ld, SENT)


def _sentinel_survives(buf: torch.Tensor, view: torch.Tensor) -> bool:
    rest = buf.clone()
    rest.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(SENT)
    return bool((rest == SENT).all())


SM, SK = 130, 128
LDA, LDW = 136, 144
# the compact call takes the same store branch as the strided one: vector when both ldr and ldc are multiples of 8
STRIDE_VARIANTS = {
    "vector": dict(N=136, ldr=152, ldc=160, cldr=136, cldc=136),
    "vector_straddling_N": dict(N=133, ldr=152, ldc=160, cldr=136, cldc=136),  # the last 8-column chunk crosses N
    "scalar_by_ldc": dict(N=132, ldr=152, ldc=141, cldr=132, cldc=132),
    "scalar_by_ldr": dict(N=132, ldr=149, ldc=160, cldr=132, cldc=132),
}


@pytest.mark.parametrize("variant", list(STRIDE_VARIANTS))
@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
def test_gemm_strides_and_padding(ln, variant):
    """nos_gemm_bf16 / nos_gemm_ln_bf16 with lda, ldw, ldr, ldc distinct and
    larger than their extents, NaN in the input padding and a sentinel in the
    C padding: bit for bit the same call on compact copies (which takes the
    same vector / scalar store branch), inside the fp64 bound, and the
    sentinel untouched everywhere outside [M, N]."""
    from nos_amd.ops import _lib

    L, st = _lib.lib(), ops._stream()
    v = STRIDE_VARIANTS[variant]
    N, M, K = v["N"], SM, SK
    if ln:
        d = _ln_gemm_data(M, N, K)
        a, w = d.x, d.wg
        ref, bound = _ln_ref(d, "gelu", 1e-5, K)
    else:
        d = _gemm_data(M, N, K)
        a, w = d.x, d.w
        ref, bound = _plain_ref(d, True, "gelu", True, K)
    (_, a_c), (_, w_c) = _place(a, K, NAN), _place(w, K, NAN)
    (_, a_s), (_, w_s) = _place(a, LDA, NAN), _place(w, LDW, NAN)
    worst = 0.0
    for policy in POLICIES:
        ops.set_gemm_policy(policy)
        try:
            (cb, c_c), (sb, c_s) = _out(M, N, v["cldc"]), _out(M, N, v["ldc"])
            if ln:
                for av, lda, wv, ldw, cv, ldc in ((a_c, K, w_c, K, c_c, v["cldc"]), (a_s, LDA, w_s, LDW, c_s, v["ldc"])):
                    rc = L.nos_gemm_ln_bf16(av.data_ptr(), lda, wv.data_ptr(), ldw, d.dc1.data_ptr(), d.dc2.data_ptr(),
                                            cv.data_ptr(), ldc, M, N, K, ops.EPI_GELU, 1e-5, 0, st)
                    assert rc == 0
            else:
                (_, r_c), (_, r_s) = _place(d.r, v["cldr"], NAN), _place(d.r, v["ldr"], NAN)
                epi = ops.EPI_BIAS | ops.EPI_GELU | ops.EPI_RESID
                for av, lda, wv, ldw, rv, ldr, cv, ldc in ((a_c, K, w_c, K, r_c, v["cldr"], c_c, v["cldc"]),
                                                           (a_s, LDA, w_s, LDW, r_s, v["ldr"], c_s, v["ldc"])):
                    rc = L.nos_gemm_bf16(av.data_ptr(), lda, wv.data_ptr(), ldw, d.db.data_ptr(), rv.data_ptr(), ldr,
                                         cv.data_ptr(), ldc, M, N, K, epi, 0, st)
                    assert rc == 0
            torch.cuda.synchronize()
        finally:
            ops.set_gemm_policy("throughput")
        worst = max(worst, _worst(c_s, ref, bound))
        assert torch.equal(_bits(c_s), _bits(c_c)), f"{policy}: strided and compact outputs differ"
        assert _sentinel_survives(sb, c_s), f"{policy}: a write outside [M, N] of the strided C"
        assert _sentinel_survives(cb, c_c), f"{policy}: a write outside [M, N] of the compact C"
    print(f"RATIO gemm_strided {'ln' if ln else 'plain'} {variant}: {worst:.3f}")
    assert worst <= 1.0, worst


PM, PN, PK = 1100, 1030, 128  # every tile kind has at least 25 tiles; with max_wg <= 8 a workgroup walks 3 or more


@pytest.mark.parametrize("kind", ["bias_gelu", "bias_residual", "ln_gelu"])
@pytest.mark.parametrize("policy", POLICIES)
def test_gemm_persistent_grids_are_bit_identical(policy, kind):
    """max_wg in {1, 3, 7, 8, 13} computes what one workgroup per tile computes.
    The kernel deals workgroup b to XCD chunk b % 8 of the tile range, so a grid
    of fewer than 8 workgroups would leave whole chunks of C unwritten: the host
    raises a cap below 8 to min(8, tiles).  The output is sentinel-filled
    first, so an unwritten tile is reported as such."""
    d = _ln_gemm_data(PM, PN, PK) if kind == "ln_gelu" else _gemm_data(PM, PN, PK)

    def run(max_wg: int) -> torch.Tensor:
        out = torch.full((PM, PN), SENT, dtype=torch.bfloat16, device=DEV)
        if kind == "ln_gelu":
            ops.linear_ln(d.dx, d.dwg, d.dc1, d.dc2, act="gelu", eps=1e-5, out=out, max_wg=max_wg)
        elif kind == "bias_gelu":
            ops.linear(d.dx, d.dw, d.db, act="gelu", out=out, max_wg=max_wg)
        else:
            ops.linear(d.dx, d.dw, d.db, residual=d.dr, out=out, max_wg=max_wg)
        return out

    ops.set_gemm_policy(policy)
    try:
        outs = {m: run(m) for m in (0, 1, 3, 7, 8, 13)}
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_policy("throughput")
    for m, y in outs.items():
        unwritten = int((y == SENT).sum())
        assert unwritten == 0, f"max_wg = {m}: {unwritten} of {PM * PN} elements of C were never written"
        assert torch.equal(_bits(y), _bits(outs[0])), f"max_wg = {m} differs from one workgroup per tile"


# ------------------------------------------------------------- B. attention
AB, AH = 2, 3
HID = AH * 64
ALD = 3 * HID + 64
ATT_BOUND = 2.0 ** -7 + 2.0 ** -11
ATT_SHAPES = ((1, 1), (1, 65), (33, 31), (64, 64), (65, 63), (127, 129), (128, 128), (129, 127), (129, 191), (257, 193),
              (100, 257), (257, 32), (40, 33))
ATT_SCALED = ((65, 63), (129, 191), (100, 257))  # also at scale = 0.05


def _attn_inputs(Sq: int, Skv: int, kind: str):
    g = torch.Generator().manual_seed(9176 * Sq + 31 * Skv + len(kind))
    q, k, v = (torch.randn(AB, s, AH, 64, generator=g) for s in (Sq, Skv, Skv))
    if kind != "flat":
        q = q * 6.0
    if kind in ("rising", "falling"):  # key norms along the sequence: the running maximum keeps / stops growing
        lo, hi = (0.2, 3.0) if kind == "rising" else (3.0, 0.2)
        k = k * torch.linspace(lo, hi, Skv).view(1, Skv, 1, 1)
    return q.bfloat16(), k.bfloat16(), v.bfloat16()


def _attn_ref(q, k, v, scale: float | None):
    scale = 0.125 if scale is None else scale
    qd, kd, vd = (t.double().transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qd @ kd.transpose(-1, -2) * scale, dim=-1)
    return (p @ vd).transpose(1, 2), ATT_BOUND * (p @ vd.abs()).transpose(1, 2), p


def _attn_run(q, k, v, scale: float | None, what: str) -> float:
    """ops.attention on views of ONE packed [B, Smax, 3*H*64 + 64] buffer whose
    K / V rows past Skv, Q rows past Sq and pad columns hold NaN (the kernel
    clamps its reads to the last valid row), into a view of a sentinel-filled
    [B, Sq + 3, H*64 + 64] buffer.  Returns the worst error / bound."""
    Sq, Skv = q.shape[1], k.shape[1]
    buf = torch.full((AB, max(Sq, Skv), ALD), NAN, dtype=torch.bfloat16)
    buf[:, :Sq, :HID] = q.flatten(2)
    buf[:, :Skv, HID:2 * HID] = k.flatten(2)
    buf[:, :Skv, 2 * HID:3 * HID] = v.flatten(2)
    buf = buf.to(DEV)
    # as_strided: a plain slice of a one-row tensor need not keep the packed row stride
    heads = lambda t, rows, col0: t.as_strided((AB, rows, AH, 64), (t.shape[1] * t.shape[2], t.shape[2], 64, 1), col0)
    qv, kv, vv = heads(buf, Sq, 0), heads(buf, Skv, HID), heads(buf, Skv, 2 * HID)
    ob = torch.full((AB, Sq + 3, HID + 64), SENT, dtype=torch.bfloat16, device=DEV)
    o = ops.attention(qv, kv, vv, scale=scale, out=heads(ob, Sq, 0))
    ref, bound, _ = _attn_ref(q, k, v, scale)
    ratio = _worst(o, ref, bound)
    assert ratio <= 1.0, (what, ratio)
    ob[:, :Sq, :HID] = SENT
    assert (ob == SENT).all(), f"{what}: a write past row Sq or into the pad columns"
    return ratio


@pytest.mark.parametrize("Sq,Skv", ATT_SHAPES)
def test_attention_shapes(Sq, Skv):
    """One key tile (wave group 1 idle), odd tile counts (group 1 skips its
    last turn), tails in the first and the second 32-key half of a tile, query
    block tails, Sq != Skv; flat, peaky (q x 6) and ramped-key inputs (the
    deferred-rescale branch, rising and falling maxima)."""
    for kind in ("flat", "peaky", "rising", "falling"):
        q, k, v = _attn_inputs(Sq, Skv, kind)
        ratio = _attn_run(q, k, v, None, kind)
        print(f"RATIO attention {kind} {Sq}x{Skv}: {ratio:.3f}")
        if (Sq, Skv) in ATT_SCALED and kind in ("flat", "peaky"):
            ratio = _attn_run(q, k, v, 0.05, kind + " scale 0.05")
            print(f"RATIO attention {kind}_scale0.05 {Sq}x{Skv}: {ratio:.3f}")


@pytest.mark.parametrize("Sq,Skv", [(129, 129), (257, 193), (300, 65), (64, 33)])
def test_attention_every_key_position_counts(Sq, Skv):
    """Query i is 3 k[j(i)] (rounded to bf16), j(i) = 7 i mod Skv -- and, in a
    second run, the LAST key for every query: the fp64 reference gives that key
    a weight of at least 0.9, so a key read from the wrong row, a masked valid
    key or a V row paired with the wrong P column moves the output by about
    0.9 |v|, a hundred times the bound."""
    _, k, v = _attn_inputs(Sq, Skv, "flat")
    for what, j in (("planted", (7 * torch.arange(Sq)) % Skv), ("last_key", torch.full((Sq,), Skv - 1))):
        q = (3.0 * k.float()[:, j]).bfloat16()
        _, _, p = _attn_ref(q, k, v, None)  # [B, H, Sq, Skv]
        weight = p.gather(-1, j.view(1, 1, Sq, 1).expand(AB, AH, Sq, 1))
        assert weight.min().item() >= 0.9, weight.min().item()
        ratio = _attn_run(q, k, v, None, what)
        print(f"RATIO attention {what} {Sq}x{Skv}: {ratio:.3f}")


def test_attention_qkv_packed_projection():
    """ops.attention_qkv (self-attention on the packed projection, the
    dispatcher's own pointer arithmetic) on a row- and batch-padded qkv."""
    S = 129
    for kind in ("flat", "peaky"):
        q, k, v = _attn_inputs(S, S, kind)
        buf = torch.full((AB, S + 2, ALD), NAN, dtype=torch.bfloat16)
        buf[:, :S, :3 * HID] = torch.cat([q.flatten(2), k.flatten(2), v.flatten(2)], dim=-1)
        buf = buf.to(DEV)
        ob = torch.full((AB, S + 3, HID + 64), SENT, dtype=torch.bfloat16, device=DEV)
        o = ops.attention_qkv(buf[:, :S, :3 * HID], AH, out=ob[:, :S, :HID])
        ref, bound, _ = _attn_ref(q, k, v, None)
        ratio = _worst(o, ref.flatten(2), bound.flatten(2))
        print(f"RATIO attention qkv_{kind} {S}x{S}: {ratio:.3f}")
        assert ratio <= 1.0, (kind, ratio)
        ob[:, :S, :HID] = SENT
        assert (ob == SENT).all()


# ------------------------------------------------------------- C. LayerNorm
LN_DS = (8, 384, 512, 520, 768, 1024, 1032, 2048, 2056, 4096)  # V = 1, 2, 4, 8: a full and a partial last vector group


def _ln_v(D: int) -> int:
    return 1 if D <= 512 else 2 if D <= 1024 else 4 if D <= 2048 else 8


@functools.lru_cache(maxsize=None)
def _ln_data(rows: int, D: int) -> SimpleNamespace:
    g = torch.Generator().manual_seed(4099 * D + rows)
    x = _kind_rows(g, rows, D, 3, period=4)  # kinds 0, 1, 2, constant (row 3), 0, 1, 2, 0, 0
    r, gamma, beta = _randn(g, rows, D), _randn(g, D), _randn(g, D)
    return SimpleNamespace(x=x, r=r, gamma=gamma, beta=beta, dx=x.to(DEV), dr=r.to(DEV), dg=gamma.to(DEV),
                           db=beta.to(DEV))


def _ln_ref64(s: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, D: int):
    s = s.double()
    mean, var = s.mean(-1, keepdim=True), s.var(-1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    gd, bd = gamma.double(), beta.double()
    ref = (s - mean) * rstd * gd + bd
    den = (s.abs() + mean.abs()) * rstd * gd.abs() + bd.abs()
    return ref, U * ref.abs() + D * F32 * den


@pytest.mark.parametrize("D", LN_DS)
def test_layernorm_every_instantiation(D):
    """All four instantiations (V = 1, 2, 4, 8 16-byte vectors per lane), 1, 5
    and 9 rows (four rows per block, with tails), with and without a residual.
    With a residual the written sum is (x + r) rounded to bf16, bit for bit,
    and the kernel normalises that rounded sum.  A constant row without a
    residual gives y == beta bit for bit (s - mean is exactly 0)."""
    worst = 0.0
    for rows in (1, 5, 9):
        d = _ln_data(rows, D)
        for eps in (1e-12, 1e-5):
            y, s = ops.layernorm(d.dx, d.dg, d.db, eps)
            assert s is None
            ref, bound = _ln_ref64(d.x, d.gamma, d.beta, eps, D)
            worst = max(worst, _worst(y, ref, bound))
            if rows > 3:
                assert torch.equal(_bits(y[3].cpu()), _bits(d.beta)), "constant row: y must equal beta"
            y, s = ops.layernorm(d.dx, d.dg, d.db, eps, residual=d.dr)
            want_s = (d.x.float() + d.r.float()).bfloat16()
            assert torch.equal(_bits(s.cpu()), _bits(want_s)), "sum_out must be bf16(x + r) bit for bit"
            ref, bound = _ln_ref64(want_s, d.gamma, d.beta, eps, D)
            worst = max(worst, _worst(y, ref, bound))
    print(f"RATIO layernorm V={_ln_v(D)} D={D}: {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("D", [384, 1032, 2056, 4096])
@pytest.mark.parametrize("resid", [False, True])
def test_layernorm_strided_views(resid, D):
    """x, residual, out and sum_out each a column slice of a wider buffer with
    its own row stride (multiples of 8, 16-byte-aligned starts), NaN around the
    inputs and a sentinel around the outputs: bit for bit the contiguous call,
    and no sentinel changes."""
    rows = 9
    d = _ln_data(rows, D)
    xb = torch.full((rows, D + 64), NAN, dtype=torch.bfloat16, device=DEV)
    rb = torch.full((rows, D + 128), NAN, dtype=torch.bfloat16, device=DEV)
    ob = torch.full((rows, D + 72), SENT, dtype=torch.bfloat16, device=DEV)
    sb = torch.full((rows, D + 40), SENT, dtype=torch.bfloat16, device=DEV)
    x, r, o, s = xb[:, 8:8 + D], rb[:, 64:64 + D], ob[:, 16:16 + D], sb[:, 24:24 + D]
    x.copy_(d.dx)
    r.copy_(d.dr)
    if resid:
        y_c, s_c = ops.layernorm(d.dx, d.dg, d.db, 1e-5, residual=d.dr)
        y_s, s_s = ops.layernorm(x, d.dg, d.db, 1e-5, residual=r, out=o, sum_out=s)
        assert s_s.data_ptr() == s.data_ptr()
        assert torch.isfinite(s_c.float()).all() and torch.equal(_bits(s), _bits(s_c))
    else:
        y_c, _ = ops.layernorm(d.dx, d.dg, d.db, 1e-5)
        y_s, s_s = ops.layernorm(x, d.dg, d.db, 1e-5, out=o)
        assert s_s is None
    assert y_s.data_ptr() == o.data_ptr()
    assert torch.isfinite(y_c.float()).all() and torch.equal(_bits(o), _bits(y_c))
    o.fill_(SENT)
    s.fill_(SENT)
    assert (ob == SENT).all() and (sb == SENT).all(), "a write outside the out / sum_out views"


def test_layernorm_host_checks():
    """Refused on the host, nothing launched: D % 8 != 0, D > 4096, a non-bf16 gamma."""
    for D in (20, 4104):
        x = torch.zeros(2, D, dtype=torch.bfloat16, device=DEV)
        gb = torch.ones(D, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(ValueError):
            ops.layernorm(x, gb, gb)
    x = torch.zeros(2, 64, dtype=torch.bfloat16, device=DEV)
    gb = torch.ones(64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        ops.layernorm(x, gb.float(), gb)


# --------------------------------------------- D. alignment contract (host side)
def _off4(rows: int, cols: int) -> torch.Tensor:
    """[rows, cols] bf16 whose rows keep a stride that is a multiple of 8 but
    whose base pointer is 8 bytes past a 16-byte boundary."""
    t = torch.zeros(rows, cols + 8, dtype=torch.bfloat16, device=DEV)[:, 4:4 + cols]
    assert t.data_ptr() % 16 == 8 and t.stride(0) % 8 == 0
    return t


def _z(*shape, dtype=torch.bfloat16) -> torch.Tensor:
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def test_linear_refuses_unaligned_base_pointers():
    """The kernels move rows as 16-byte vectors (LDS-DMA, vector loads and
    stores); a column slice such as x[:, 4:4 + K] passes every stride check.
    The wrappers raise before anything is launched."""
    M, N, K = 16, 32, 64
    x, w, b, r = _z(M, K), _z(N, K), _z(N), _z(M, N)
    for kw in (dict(x=_off4(M, K)), dict(weight=_off4(N, K)), dict(residual=_off4(M, N)), dict(out=_off4(M, N))):
        args = dict(x=x, weight=w, bias=b, residual=r, out=None)
        args.update(kw)
        with pytest.raises(ValueError, match="16-byte"):
            ops.linear(args["x"], args["weight"], args["bias"], residual=args["residual"], out=args["out"])
    c1, c2 = _z(N, dtype=torch.float32), _z(N, dtype=torch.float32)
    for kw in (dict(x=_off4(M, K)), dict(wg=_off4(N, K)), dict(out=_off4(M, N))):
        args = dict(x=x, wg=w, out=None)
        args.update(kw)
        with pytest.raises(ValueError, match="16-byte"):
            ops.linear_ln(args["x"], args["wg"], c1, c2, out=args["out"])


def test_attention_refuses_unaligned_base_pointers():
    B, S = 1, 16
    good = _z(B, S, 3 * HID)
    bad = _z(B, S, 3 * HID + 8)[..., 4:4 + 3 * HID]
    assert bad.data_ptr() % 16 == 8
    out_bad = _z(B, S, HID + 8)[..., 4:4 + HID]
    with pytest.raises(ValueError, match="16-byte"):
        ops.attention_qkv(bad, AH)
    with pytest.raises(ValueError, match="16-byte"):
        ops.attention_qkv(good, AH, out=out_bad)
    split = lambda t: [t[..., i * HID:(i + 1) * HID].unflatten(-1, (AH, 64)) for i in range(3)]
    with pytest.raises(ValueError, match="16-byte"):
        ops.attention(*split(bad))
    with pytest.raises(ValueError, match="16-byte"):
        ops.attention(*split(good), out=out_bad.unflatten(-1, (AH, 64)))


def test_layernorm_refuses_unaligned_base_pointers():
    rows, D = 4, 64
    x, g = _z(rows, D), _z(D)
    g_bad = _z(D + 8)[4:4 + D]
    assert g_bad.is_contiguous() and g_bad.data_ptr() % 16 == 8
    for kw in (dict(x=_off4(rows, D)), dict(gamma=g_bad), dict(beta=g_bad), dict(residual=_off4(rows, D)),
               dict(out=_off4(rows, D)), dict(sum_out=_off4(rows, D))):
        args = dict(x=x, gamma=g, beta=g, residual=x, out=None, sum_out=None)
        args.update(kw)
        with pytest.raises(ValueError, match="16-byte"):
            ops.layernorm(args["x"], args["gamma"], args["beta"], 1e-5, residual=args["residual"], out=args["out"],
                          sum_out=args["sum_out"])
