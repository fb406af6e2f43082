"""Edges of the general tenant ops (nos_amd/ops/tenant.py over
csrc/hip/tenant_ops.hip, attention_h3g.hip, attention_h3g_bwd.hip) that
tests/test_tenant_ops_gpu.py and test_flash_attention_train_gpu.py never pass:
widths around the 64-lane wave, -inf / NaN / +inf rows of the softmax, row
strides, conv kernels with nothing square, and the attention family's
``scale``, ``rope`` with Sq < Skv, ``out=``, key splits at Sq != Skv and
all-zero operands.

Criteria (the suite's own, none invented here):

* fp32 results: ``_close_to_fp64`` of test_tenant_ops_gpu.py -- the error
  against fp64 is at most max(4 x torch-fp32's error, 5e-6), both references
  plain torch ops on the GPU;
* backward: ``_check`` of test_flash_attention_train_gpu.py (4 x, floor 1e-5),
  copied here with the output names as an argument so that an output the
  case states to be exactly zero is compared with ``torch.equal`` instead;
* bf16 outputs of kernels that round once (softmax, rotary, glu): within one
  bf16 ulp of the fp64 result rounded to bf16, ``|got - ref_b| <= 2^-7 |ref_b|``
  (an fp32 value a few fp32 ulps from the truth rounds to the same or the
  adjacent bf16); rmsnorm rounds twice, as HF does: two ulps, ``2^-6 |ref_b|``.

Every check prints its figures before it asserts (``pytest -s``): the lines
``RATIO <group> ...`` give error / bound, the baseline of a later tightening."""
from __future__ import annotations

import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from nos_amd.ops import tenant as T  # noqa: E402
from nos_amd.podserver.program.reference import sdpa_cache_ref  # noqa: E402
from test_tenant_ops_gpu import _close_to_fp64, _err, _rope_tables  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
NINF = float("-inf")


@pytest.fixture(autouse=True)
def _no_tf32():
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    yield
    T.set_attention_h3g_kvsplit(0)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


# ------------------------------------------------------------------ criteria
def _fp32_ok(group: str, what, got, ref64, f32):
    """``_close_to_fp64`` with the figures printed first."""
    assert got.shape == ref64.shape and got.dtype == torch.float32, (got.shape, got.dtype)
    assert torch.isfinite(got).all(), what
    e, e32 = _err(got, ref64), _err(f32, ref64)
    print(f"RATIO {group} {what}: err {e:.3e} torch-fp32 {e32:.3e} err/bound {e / max(4 * e32, 5e-6):.3f}")
    _close_to_fp64(got, ref64, f32)


def _bf16_ok(group: str, what, got, ref64, ulps: int = 1):
    """got (bf16) within ``ulps`` bf16 ulps of ref64 rounded to bf16: |got - ref_b| <= ulps 2^-8 ... 2^-7 |ref_b|,
    taken at its upper end 2^-7 (one ulp) / 2^-6 (two)."""
    assert got.dtype == BF16 and got.shape == ref64.shape
    ref_b = ref64.to(BF16).double()
    d = (got.double() - ref_b).abs()
    worst = float((d / ref_b.abs().clamp_min(1e-300)).nan_to_num(0.0).max())
    print(f"RATIO {group} {what}: bf16 worst |got - ref_b| / |ref_b| {worst:.3e} = {worst * 2 ** 8:.2f} x 2^-8")
    assert bool((d <= ulps * 2.0 ** -7 * ref_b.abs()).all()), (what, worst)


def _row_ok(group, what, got, ref64, f32, ulps: int = 1):
    if got.dtype == BF16:
        _bf16_ok(group, what, got, ref64, ulps)
    else:
        _fp32_ok(group, what, got, ref64, f32)


# the backward's criterion: test_flash_attention_train_gpu.py _rel / _check, the names an argument
def _rel(a, b, zero_den: float) -> float:
    den = float(b.double().abs().max())
    return float((a.double() - b.double()).abs().max()) / (den if den > 0 else zero_den)


def _check(group, what, names, ours, r64, r32, dens=None):
    dens = dens or {}
    for name in names:
        a, b, c, zd = ours[name], r64[name], r32[name], dens.get(name, 1.0)
        assert a.shape == b.shape and torch.isfinite(a).all(), (what, name)
        ea, ec = _rel(a, b, zd), _rel(c, b, zd)
        print(f"RATIO {group} {what} {name}: rel {ea:.3e} torch-fp32 {ec:.3e} err/bound {ea / max(4 * ec, 1e-5):.3f}")
        assert ea <= max(4 * ec, 1e-5), (what, name, ea, ec)


# ================================================================== A. softmax
SOFTMAX_L = [1, 2, 63, 64, 65, 127, 128, 129, 200, 4099]


@pytest.mark.parametrize("L", SOFTMAX_L)
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_softmax_widths_around_the_wave(dt, L):
    for rows in (1, 5):   # 5: the last 4-row block is partly empty
        x = (_randn(_gen(10 + L + rows), rows, L) * 3).to(dt)
        got = T.softmax(x)
        assert got.shape == x.shape and got.dtype == dt
        _row_ok("A", f"softmax L={L} rows={rows}", got, torch.softmax(x.double(), -1), torch.softmax(x.float(), -1))


def _neg_inf_rows(dt):
    L = 200
    x = (_randn(_gen(11), 6, L) * 3).to(dt)
    mask = torch.zeros(6, L, dtype=torch.bool, device="cuda")
    mask[0, :70] = True            # the first column of every lane, and the second of lanes 0..5
    mask[1, 5] = True
    mask[2, 0::2] = True
    mask[3, :L - 1] = True         # one column left
    mask[4, 150:] = True           # the causal pattern
    mask[5, :] = True              # nothing left: NaN, as torch
    return x.masked_fill(mask, NINF), mask


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_softmax_masked_columns(dt):
    """-inf columns in front of, between and behind finite ones.  The kernel
    before this test failed it: a lane that met -inf before any finite value
    carried exp(-inf - -inf) = NaN into the wave sum, and rows 0, 1 and 3
    came out as 200 NaNs each (NaNs per row [200, 200, 0, 200, 0, 200])."""
    x, mask = _neg_inf_rows(dt)
    got = T.softmax(x)
    ref = torch.softmax(x.float(), -1)
    print("NaNs per row:", torch.isnan(got).sum(-1).tolist(), "torch:", torch.isnan(ref).sum(-1).tolist())
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert bool(torch.isnan(got[5]).all()) and not bool(torch.isnan(got[:5]).any())
    _row_ok("A", "softmax -inf rows", got[:5], torch.softmax(x[:5].double(), -1), ref[:5])
    assert torch.equal(got[:5][mask[:5]], torch.zeros_like(got[:5][mask[:5]]))
    assert torch.equal(got[3], F.one_hot(torch.tensor(199, device="cuda"), 200).to(dt))


@pytest.mark.parametrize("L", [5, 200])   # 5: the non-finite value is all its lane sees
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_softmax_non_finite_rows_as_torch(dt, L):
    x = (_randn(_gen(12), 3, L) * 3).to(dt)
    x[0, L // 2] = float("inf")
    x[1, 3] = float("nan")
    x[2, 1] = NINF
    got = T.softmax(x)
    ref = torch.softmax(x.float(), -1)
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert bool(torch.isnan(got[:2]).all()) and bool(torch.isfinite(got[2]).all())


def test_softmax_fp32_large_offset_and_constant_row():
    x = _randn(_gen(13), 5, 200) * 30 + 1e4   # the row maximum is subtracted: no overflow
    _fp32_ok("A", "softmax 1e4 offset", T.softmax(x), torch.softmax(x.double(), -1), torch.softmax(x, -1))
    for L in (1, 64, 200, 4099):
        c = torch.full((2, L), -7.25, device="cuda")
        got = T.softmax(c)
        _fp32_ok("A", f"softmax constant L={L}", got, torch.full_like(c, 1.0 / L, dtype=torch.float64), torch.softmax(c, -1))


@pytest.mark.parametrize("L", [65, 200])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_softmax_reads_strided_rows(dt, L):
    wide = (_randn(_gen(14), 5, L + 11) * 3).to(dt)
    x = wide[:, 3:3 + L]
    assert x.stride(0) != L and x.stride(1) == 1
    assert torch.equal(T.softmax(x), T.softmax(x.contiguous()))


# ================================================================== B. rmsnorm, rotary, embedding, glu
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("D", [1, 8, 63, 64, 65, 200, 4100])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_rmsnorm_widths_eps_and_row_scales(dt, D, eps):
    for rows in (1, 5):
        g = _gen(20 + D + rows)
        scales = torch.tensor([1e-3, 1.0, 1e3, 1.0, 1e-3], device="cuda")[:rows, None]   # 1e-3: eps is part of the result
        x = (_randn(g, rows, D) * scales).to(dt)
        w = (1 + 0.1 * _randn(g, D)).to(dt)
        got = T.rmsnorm(x, w, eps)
        assert got.shape == x.shape and got.dtype == dt
        _row_ok("B", f"rmsnorm D={D} rows={rows} eps={eps}", got, T.rmsnorm_ref(x.double(), w.double(), eps),
                T.rmsnorm_ref(x.float(), w.float(), eps), ulps=2)


@pytest.mark.parametrize("D", [65, 200])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_rmsnorm_reads_strided_rows(dt, D):
    g = _gen(21)
    wide = (_randn(g, 5, D + 11) * 3).to(dt)
    w = (1 + 0.1 * _randn(g, D)).to(dt)
    x = wide[:, 3:3 + D]
    assert x.stride(0) != D
    assert torch.equal(T.rmsnorm(x, w, 1e-5), T.rmsnorm(x.contiguous(), w, 1e-5))


@pytest.mark.parametrize("S", [1, 9])
@pytest.mark.parametrize("D", [2, 64, 128])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_rotary_on_a_fused_projection_slice(dt, D, S):
    B, H = 2, 3
    qkv = _randn(_gen(22 + D + S), B, S, (H + 2) * D).to(dt)
    x = qkv[..., :H * D].view(B, S, H, D)
    assert not x.is_contiguous()
    c, s = _rope_tables(S + 4, D)   # more table rows than tokens
    got = T.rotary(x, c, s)
    assert got.shape == (B, S, H, D) and got.dtype == dt and got.is_contiguous()
    _row_ok("B", f"rotary D={D} S={S}", got, T.rope_ref(x.double(), c.double(), s.double()), T.rope_ref(x.float(), c, s))


@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("tdt,D", [(F32, 4), (F32, 128), (BF16, 8)], ids=["f32x4", "f32x128", "bf16x8"])
def test_embedding_invalid_ids_give_zero_rows(tdt, D, idt):
    V = 11
    table = (_randn(_gen(23), V, D) + 3).to(tdt)   # + 3: no row of the table is zero
    for ids in ([-1, 0, V - 1, V, 3, 3, 0], [[-1, 0, V - 1], [V, 3, 3]], [V - 1], [-1], [V]):
        it = torch.tensor(ids, dtype=idt, device="cuda")
        got = T.embedding(it, table)
        assert got.shape == (*it.shape, D) and got.dtype == tdt
        ok = (it >= 0) & (it < V)
        assert torch.equal(got[ok], table[it[ok].long()])
        assert torch.equal(got[~ok], torch.zeros_like(got[~ok]))


_GLU_F = {"relu": F.relu, "sigmoid": torch.sigmoid, "silu": F.silu, "gelu": F.gelu}


@pytest.mark.parametrize("op", list(_GLU_F))
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_glu_on_the_halves_of_a_merged_projection(dt, op):
    f = _GLU_F[op]
    for M in (1, 5):
        for N in (1, 7, 2816):
            t = _randn(_gen(24 + M + N), M, 2 * N).to(dt)
            a, b = t[:, :N], t[:, N:]
            assert a.stride(0) == 2 * N and b.stride(0) == 2 * N
            got = T.glu(a, b, op)
            assert got.shape == (M, N) and got.dtype == dt and got.is_contiguous()
            _row_ok("B", f"glu {op} M={M} N={N}", got, f(a.double()) * b.double(), f(a.float()) * b.float())


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_glu_reads_a_and_b_at_their_own_row_strides(dt):
    """a and b from two projections of different widths: b read at a's stride would go unseen above."""
    g = _gen(26)
    for N in (7, 70):
        a, b = _randn(g, 5, 2 * N).to(dt)[:, :N], _randn(g, 5, 3 * N).to(dt)[:, N:2 * N]
        assert a.stride(0) == 2 * N and b.stride(0) == 3 * N
        _row_ok("B", f"glu silu strides N={N}", T.glu(a, b, "silu"), F.silu(a.double()) * b.double(),
                F.silu(a.float()) * b.float())


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_glu_contiguous_3d(dt):
    g = _gen(25)
    a, b = _randn(g, 2, 3, 70).to(dt), _randn(g, 2, 3, 70).to(dt)
    _row_ok("B", "glu silu contiguous", T.glu(a, b, "silu"), F.silu(a.double()) * b.double(), F.silu(a.float()) * b.float())


# ================================================================== C. conv2d with nothing square
CONVS = [  # (kh, kw), stride, padding, dilation
    ((1, 7), (1, 1), (0, 3), (1, 1)),
    ((7, 1), (2, 1), (3, 0), (1, 1)),
    ((3, 5), (1, 3), (2, 0), (1, 2)),
    ((2, 3), (2, 2), (0, 1), (2, 1)),
    ((3, 3), (1, 2), (1, 0), (2, 1)),   # the templated 3x3 path
    ((7, 7), (2, 1), (3, 2), (1, 1)),   # the templated 7x7 path
]


def _conv_case(group, what, n, c, oc, ks, st, pd, dl, groups=1):
    g = _gen(30)
    x = _randn(g, n, c, 13, 17)
    w = _randn(g, oc, c // groups, *ks) / math.sqrt(c // groups * ks[0] * ks[1])
    b = _randn(g, oc)
    ref64 = F.conv2d(x.double(), w.double(), b.double(), st, pd, dl, groups)
    got = T.conv2d(x, w, b, st, pd, dl, groups=groups)
    _fp32_ok(group, what, got, ref64, F.conv2d(x, w, b, st, pd, dl, groups))


@pytest.mark.parametrize("ks,st,pd,dl", CONVS, ids=[f"k{k[0]}x{k[1]}" for k, *_ in CONVS])
def test_conv2d_rectangular_kernels_and_unequal_strides(ks, st, pd, dl):
    """kh != kw, and strides / paddings / dilations that differ per axis: the
    im2col's (c, i, j) split and its (ih, iw) arithmetic cannot swap axes unseen."""
    _conv_case("C", f"conv2d k={ks} s={st} p={pd} d={dl}", 2, 5, 6, ks, st, pd, dl)


def test_grouped_conv2d_rectangular_kernel():
    """Depthwise over the 5 channels (10 output channels: a multiple of the groups)."""
    _conv_case("C", "conv2d grouped k=(3, 5) s=(2, 1)", 2, 5, 10, (3, 5), (2, 1), (1, 2), (1, 1), groups=5)


# ================================================================== D. attention arguments
B, HKV, G = 2, 2, 2
H = HKV * G
NAMES = ("o", "dq", "dk", "dv")


def _qkvdo(D, sq, skv, seed=0):
    g = _gen(40 + seed + 131 * D + sq + 7 * skv)
    return _randn(g, B, sq, H, D), _randn(g, B, skv, HKV, D), _randn(g, B, skv, HKV, D), _randn(g, B, sq, H, D)


def _autograd(q, k, v, do, causal, scale):
    """o, dq, dk, dv of plain torch ops (autograd) in the inputs' dtype."""
    xs = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    s = T._train_scores(xs[0], xs[1], causal, scale)
    y = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), xs[2].repeat_interleave(q.shape[2] // k.shape[2], dim=2))
    y.backward(do.to(y.dtype))
    return dict(zip(NAMES, [y.detach()] + [t.grad for t in xs]))


def _lse(q, k, causal, scale):
    return torch.logsumexp(T._train_scores(q, k, causal, scale), -1)


def _refs(q, k, v, do, causal, scale):
    """(fp64, torch-fp32) autograd results and log-sum-exps of one case."""
    q64, k64, v64, do64 = (t.double() for t in (q, k, v, do))
    r64, r32 = _autograd(q64, k64, v64, do64, causal, scale), _autograd(q, k, v, do, causal, scale)
    r64["lse"], r32["lse"] = _lse(q64, k64, causal, scale), _lse(q, k, causal, scale)
    return r64, r32


@functools.lru_cache(maxsize=None)
def _case(D, causal, sq, skv, scale):
    """Inputs and both references: computed once, shared, never written."""
    x = _qkvdo(D, sq, skv)
    return x, *_refs(*x, causal, scale)


def _lse_ok(group, what, lse, r64, r32):
    """The log-sum-exp's bound of test_flash_attention_train_gpu.py: absolute, 4 x torch fp32's, floor 1e-5."""
    assert lse.shape == r64["lse"].shape and lse.dtype == F32
    e = float((lse.double() - r64["lse"]).abs().max())
    e32 = float((r32["lse"].double() - r64["lse"]).abs().max())
    print(f"RATIO {group} {what} lse: err {e:.3e} torch-fp32 {e32:.3e} err/bound {e / max(4 * e32, 1e-5):.3f}")
    assert e <= max(4 * e32, 1e-5), (what, e, e32)


def _fwd_bwd(q, k, v, do, causal, scale=None):
    o, lse = T.sdpa_lse(q, k, v, causal, scale)
    return dict(zip(NAMES, (o, *T.sdpa_bwd(q, k, v, o, lse, do, causal, scale)))), lse


@pytest.mark.parametrize("scale", [0.03, 1.0])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_attention_scale_forward_and_backward(D, causal, scale):
    """``scale`` away from D^-0.5 through sdpa, sdpa_lse and sdpa_bwd (c = scale log2 e,
    the two dS factors and the dS bound), single-pass and with key splits."""
    (q, k, v, do), r64, r32 = _case(D, causal, 40, 72, scale)
    for split in (0, 2):
        T.set_attention_h3g_kvsplit(split)
        what = f"scale={scale} D={D} causal={causal} split={split}"
        o = T.sdpa(q, k, v, causal=causal, scale=scale)
        _fp32_ok("D", "sdpa " + what, o, r64["o"], r32["o"])
        ours, lse = _fwd_bwd(q, k, v, do, causal, scale)
        assert torch.equal(ours["o"], o)
        _lse_ok("D", what, lse, r64, r32)
        _check("D", what, NAMES, ours, r64, r32)


@pytest.mark.parametrize("scale", [0.03, 1.0])
@pytest.mark.parametrize("Sq", [1, 5])
@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_scale(D, Sq, scale):
    L = 300
    g = _gen(41 + D + Sq)
    kc, vc, q = _randn(g, B, L, HKV, D), _randn(g, B, L, HKV, D), _randn(g, B, Sq, H, D)
    pos = torch.tensor([7, L - Sq], dtype=torch.int32, device="cuda")   # the second sequence ends on the last key
    qc, kcc, vcc, pc = q.cpu(), kc.cpu(), vc.cpu(), pos.cpu()
    ref64 = sdpa_cache_ref(qc.double(), kcc.double(), vcc.double(), pc, scale)
    assert ref64.dtype == torch.float64
    ref32 = sdpa_cache_ref(qc, kcc, vcc, pc, scale)
    for split in (0, 2):
        T.set_attention_h3g_kvsplit(split)
        got = T.sdpa_cache(q, kc, vc, pos, scale)
        _fp32_ok("D", f"sdpa_cache scale={scale} D={D} Sq={Sq} split={split}", got.cpu(), ref64, ref32)


@pytest.mark.parametrize("sq,skv", [(40, 72), (1, 300)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_rope_rotates_queries_at_the_end_of_the_keys(D, causal, sq, skv):
    """Sq < Skv: query row i is rotated at position i + Skv - Sq."""
    q, k, v, _ = _qkvdo(D, sq, skv, seed=1)
    k = k * 2
    c, s = _rope_tables(skv, D)
    ref64 = T.sdpa_ref(q.double(), k.double(), v.double(), causal, None, (c.double(), s.double()))
    assert ref64.dtype == torch.float64
    f32 = T.sdpa_ref(q, k, v, causal, None, (c, s))
    for split in (0, 3):
        T.set_attention_h3g_kvsplit(split)
        got = T.sdpa(q, k, v, causal=causal, rope=(c, s))
        _fp32_ok("D", f"rope {sq}x{skv} D={D} causal={causal} split={split}", got, ref64, f32)


@pytest.mark.parametrize("nsplit", [1, 2, 3, 4])
@pytest.mark.parametrize("D,causal,sq,skv", [(64, True, 40, 300), (128, True, 40, 300), (64, False, 77, 77)])
def test_key_splits_with_fewer_queries_than_keys(D, causal, sq, skv, nsplit):
    (q, k, v, _), r64, r32 = _case(D, causal, sq, skv, D ** -0.5)
    T.set_attention_h3g_kvsplit(nsplit)
    what = f"splits={nsplit} {sq}x{skv} D={D} causal={causal}"
    o = T.sdpa(q, k, v, causal=causal)
    _fp32_ok("D", what, o, r64["o"], r32["o"])
    o2, lse = T.sdpa_lse(q, k, v, causal)
    assert torch.equal(o2, o)
    _lse_ok("D", what, lse, r64, r32)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_sdpa_out_strided_and_bf16(D, causal):
    q, k, v, _ = _qkvdo(D, 40, 72, seed=2)
    for split in (0, 2):
        T.set_attention_h3g_kvsplit(split)
        plain = T.sdpa(q, k, v, causal=causal)
        buf = torch.full((B, 40, H * D + 32), float("nan"), device="cuda")
        out = buf[..., 16:16 + H * D].view(B, 40, H, D)
        assert out.stride(1) == H * D + 32 and out.data_ptr() == buf.data_ptr() + 64
        ret = T.sdpa(q, k, v, causal=causal, out=out)
        assert ret is out and torch.equal(out, plain)
        assert bool(torch.isnan(buf[..., :16]).all()) and bool(torch.isnan(buf[..., 16 + H * D:]).all())
        o16 = torch.empty((B, 40, H, D), dtype=BF16, device="cuda")
        ret = T.sdpa(q, k, v, causal=causal, out=o16)
        assert ret is o16 and torch.equal(o16, plain.to(BF16))


def _zero_case(D, causal, sq, skv, what, edit, zeros):
    """One zeroed operand: everything finite, the outputs in ``zeros`` exactly
    zero (here and in fp64), the others under the backward's criterion."""
    q, k, v, do = (t.clone() for t in _qkvdo(D, sq, skv, seed=3))
    edit(q, k, v, do)
    r64, r32 = _refs(q, k, v, do, causal, D ** -0.5)
    ours, lse = _fwd_bwd(q, k, v, do, causal)
    for name in NAMES:
        assert torch.isfinite(ours[name]).all(), (what, name)
    assert torch.isfinite(lse).all(), what
    for name in zeros:
        assert not r64[name].any(), (what, name)   # the reference agrees that it is zero
        assert torch.equal(ours[name], torch.zeros_like(ours[name])), (what, name)
    what = f"{what} {sq}x{skv} D={D} causal={causal}"
    _check("D", what, [n for n in NAMES if n not in zeros], ours, r64, r32)
    _lse_ok("D", what, lse, r64, r32)
    return ours, (q, k, v, do)


ZEROS = {
    "K=0": (lambda q, k, v, do: k.zero_(), ("dq",)),
    "V=0": (lambda q, k, v, do: v.zero_(), ("o", "dq", "dk")),
    "dO=0": (lambda q, k, v, do: do.zero_(), ("dq", "dk", "dv")),
    "Q=0": (lambda q, k, v, do: q.zero_(), ("dk",)),   # dk = dS^T Q: identically zero in fp64 too
    "one dO row, one K head": (lambda q, k, v, do: (do[1, 7].zero_(), k[:, :, 1].zero_()), ()),
}


@pytest.mark.parametrize("which", list(ZEROS))
@pytest.mark.parametrize("sq,skv", [(33, 33), (40, 72)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_attention_zero_operands(D, causal, sq, skv, which):
    """The abs-max scales of an all-zero operand (h3_scale_exp(0), the dS
    bound's exponent, 1 / the K / V scale) give zeros, never inf or NaN."""
    edit, zeros = ZEROS[which]
    ours, (q, k, v, do) = _zero_case(D, causal, sq, skv, which, edit, zeros)
    if which == "K=0":   # equal scores: o is the mean of the values a row sees
        vm = v.double().repeat_interleave(G, dim=2)
        if causal:
            n = torch.arange(1, sq + 1, device="cuda", dtype=torch.float64) + (skv - sq)
            mean = vm.cumsum(1)[:, skv - sq:] / n[None, :, None, None]
        else:
            mean = vm.mean(1, keepdim=True).expand(B, sq, H, D)
        _fp32_ok("D", f"K=0 mean of V {sq}x{skv} D={D} causal={causal}", ours["o"], mean,
                 T.sdpa_ref(q, k, v, causal))
    if which == "one dO row, one K head":
        assert torch.equal(ours["dq"][:, :, G:2 * G], torch.zeros_like(ours["dq"][:, :, G:2 * G]))   # dq = dS K, K head 1 = 0


# ================================================================== E. rope with Sq > Skv
@pytest.mark.parametrize("causal", [False, True])
def test_rope_with_more_queries_than_keys_is_refused(causal):
    """Query row i would be rotated at table row i + Skv - Sq < 0: refused
    before the library is touched (nothing is launched)."""
    q = torch.zeros(1, 40, 2, 64, device="cuda")
    k = torch.zeros(1, 33, 1, 64, device="cuda")
    c, s = _rope_tables(33, 64)
    with pytest.raises(ValueError, match="rope needs Sq <= Skv"):
        T.sdpa(q, k, k, causal=causal, rope=(c, s))
