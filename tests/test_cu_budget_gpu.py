"""The persistent form of every kernel a CU-mask slice pod runs by default.

A slice pod calls ``ops.set_cu_budget(popcount of its mask)``; every item-loop
kernel then launches at most occupancy x budget workgroups (a multiple of 8,
csrc/hip/runtime.hip ``nos_grid_for``) that each WALK several items of their
XCD's chunk (``nos::xcd_chunk``).  The second pass of that loop -- the LDS ring
and the C tile held in it reused, the DMA counts, accumulators and per-item
constants re-initialised, the barrier between items, a chunk with an uneven
tail -- runs nowhere else.  Here: the h3 GEMM in its three modes and every
epilogue, the head-dim-64 h3 attention, the general h3 attention forward and
backward, and the int8 GEMV / dequantization, at budgets 8 and 20.

A tile's arithmetic does not depend on the workgroup that runs it, so wherever
the budget leaves the number of key splits / sweep ranges alone the budgeted
result equals the unbudgeted one BIT FOR BIT; where the budget changes that
number (``pick_split`` in auto mode, the backward's sweep ranges) the result
is compared with fp64 under the criterion of that kernel's own test.

Every case has more items than a budget of 8 can hold at once whatever
occupancy the runtime reports: a CU holds at most 32 waves, so 8 CUs hold at
most 8 x 8 = 64 workgroups of 256 threads or 8 x 4 = 32 of 512 threads (the
arithmetic stands next to each shape).  Outputs are caller-allocated and
pre-filled with NaN (fp16 0x7E00 in planes), workspaces that carry partials
with 0xFF bytes, and every output must be finite before it is compared: an
item nobody ran cannot pass on the right values left in recycled memory."""
from __future__ import annotations

import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402
from nos_amd.ops import _lib, _stream  # noqa: E402
from nos_amd.ops import tenant as T  # noqa: E402

BUDGETS = (8, 20)   # 8: the guaranteed walk; 20: another grid, XCD chunks of 10 and 11 items on another stride
EPI_BIAS, EPI_GELU, EPI_RESID, EPI_BIAS_ROW = 1, 2, 4, 16
EPS = 1e-6
NAN16 = 0x7E00      # fp16 NaN


@pytest.fixture(autouse=True)
def _slice_pod_config():
    """A slice pod's kernel configuration (models/pod.py ``kernel_config``: h3
    math, LDS epilogue, 2-deep hot ring, 128-wide hot tiles) for every test;
    whatever a test switches is put back.  The library has no getter for the
    LDS epilogue and the hot ring: they return to its defaults (on, 2)."""
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = (ops.f32_math(), ops.attention_f32_variant(), ops._LN_HANDOFF, ops.stats_pw())
    assert ops.cu_budget() == 0
    ops.set_f32_math("h3")
    ops.set_attention_f32_variant("h3n")
    ops.set_ln_handoff(False)
    ops.set_gemm_f32h3_lds_epilogue(True)
    ops.set_gemm_f32h3_hot_ring(2)
    ops.set_gemm_f32h3_hot_bn(128)
    try:
        yield
    finally:
        ops.set_cu_budget(0)
        ops.set_f32_math(prev[0])
        ops.set_attention_f32_variant("h3")   # a forced "h3k2" split back to auto
        ops.set_attention_f32_variant(prev[1])
        ops.set_ln_handoff(prev[2])
        ops.set_gemm_f32h3_lds_epilogue(True)
        ops.set_gemm_f32h3_hot_ring(2)
        ops.set_gemm_f32h3_hot_bn(prev[3])
        T.set_attention_h3g_kvsplit(0)


@pytest.fixture
def poisoned_workspaces(monkeypatch):
    """The scratch of T.sdpa / T.sdpa_bwd (key-split partials, partial dK / dV) filled with 0xFF bytes: NaN
    in every format, so a partial nobody wrote cannot be a stale right value of the run before."""
    def workspace(nbytes, device):
        ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=device)
        return ws, (ws.data_ptr() + 255) // 256 * 256

    monkeypatch.setattr(T, "_workspace", workspace)
    return workspace


def _nan32(*shape) -> torch.Tensor:
    return torch.full(shape, math.nan, dtype=torch.float32, device="cuda")


def _nan16(*shape) -> torch.Tensor:
    return torch.full(shape, NAN16, dtype=torch.int16, device="cuda").view(torch.float16)


def _values(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.float16) if t.dtype == torch.int16 else t


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _under(budget: int, run):
    ops.set_cu_budget(budget)
    try:
        outs = run()
        torch.cuda.synchronize()
    finally:
        ops.set_cu_budget(0)
    return outs


def _assert_written(outs: dict, what) -> None:
    for name, t in outs.items():
        bad = int((~torch.isfinite(_values(t).float())).sum())
        assert bad == 0, f"{what} {name}: {bad} of {t.numel()} elements unwritten (NaN pre-fill) or not finite"


def _assert_same_bits(ref: dict, got: dict, what) -> None:
    assert ref.keys() == got.keys()
    for name in ref:
        a, b = _bits(ref[name]), _bits(got[name])
        if not torch.equal(a, b):
            d = (_values(ref[name]).double() - _values(got[name]).double()).abs().max().item()
            raise AssertionError(f"{what} {name}: {int((a != b).sum())} of {a.numel()} elements differ from the "
                                 f"reference run, max |difference| {d:.3e}")


def _bit_identical_under_budgets(run, what="") -> dict:
    """run() -> {name: freshly NaN-filled output}: complete and equal to budget 0 bit for bit at every budget."""
    ref = _under(0, run)
    _assert_written(ref, f"{what} budget 0")
    for budget in BUDGETS:
        got = _under(budget, run)
        _assert_written(got, f"{what} budget {budget}")
        _assert_same_bits(ref, got, f"{what} budget {budget}")
    return ref


# ------------------------------------------------------------------ 1. the h3 GEMM
# M = 1100, K = 96: 9 row tiles of 128 (the last one 76 rows) and three K stages of 32.  128 x 128 tiles
# of 256 threads: at most 64 workgroups at budget 8.
#   N = 1028: 9 column tiles (the last 4 wide),   81 tiles > 64   (128 x 64 hot tiles: 17 x 9 = 153)
#   N = 1030: 9 column tiles (the last 6 wide),   81 tiles > 64
#   N = 1032: 9 column tiles (the last 8 wide),   81 tiles > 64
#   N = 1152 = 3 x 6 x 64 (QKV of 6 heads):       81 tiles > 64
M, K = 1100, 96


@pytest.fixture(scope="module")
def gemm():
    g = torch.Generator(device="cuda").manual_seed(1100)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    d = {"x": rn(M, K) * 2 + 0.5}
    for N in (1028, 1030, 1032, 1152):
        w = rn(N, K) / K ** 0.5
        d[N] = (w, rn(N) * 0.5, rn(M, N), w.sum(1))      # weight, bias (c2), residual, c1
    # a pre-LN residual GEMM that produces [M, K] rows with their statistics (case e)
    d["producer"] = (rn(M, 64), rn(K, 64) / 8, rn(K), rn(M, K) * 3 + 2)
    torch.cuda.synchronize()
    return d


def _linear(x, w, b, act, res) -> torch.Tensor:
    out = _nan32(M, w.shape[0])
    ops.linear(x, w, b, act=act, residual=res, out=out)
    return out


def _linear_ln(x, w, b, c1, act, pre=None) -> torch.Tensor:
    out = _nan32(M, w.shape[0])
    ops.linear_ln(x, w, c1, b, act=act, eps=EPS, out=out, pre=pre)
    return out


def _ln_to_planes(x, w, b, pre=None) -> torch.Tensor:
    """fc1 -> fc2 (ops.linear_ln_to_planes, one level down): GELU(LN(x) W^T + b) as the next GEMM's A planes."""
    planes = _nan16(2, M, w.shape[0])
    ops._gemm_ln_h3(x, pre, EPS, w, b, None, EPI_BIAS | EPI_GELU, planes_out=(planes, ops._h3_out_scale(w, b, "gelu")))
    return planes


def _ln_qkv(x3, w, b, H, pre=None):
    """ops.linear_ln_qkv_h3 one level down: (qkv whose Q columns are written, the attention's workspace, scales)."""
    B, S, k = x3.shape
    N = w.shape[0]
    qkv = _nan32(B, S, N)
    ws = torch.full((int(_lib.lib().nos_attn_f32x6_workspace(B, H, S, S)) // 2,), NAN16, dtype=torch.int16,
                    device="cuda")
    sc = ops.h3_head_scales(w, b, H)
    ops._gemm_ln_h3(x3.reshape(-1, k), pre, EPS, w, b, qkv.view(-1, N), EPI_BIAS, kv=(ws, S, (S + 31) // 32 * 32, sc))
    return qkv, ws, sc


def _qkv_outputs(qkv, ws, H) -> dict:
    """What the projection must have written: the Q columns, and every plane row of a real token."""
    B, S, N = qkv.shape
    hd, skvp = N // 3, (S + 31) // 32 * 32
    return {"q": qkv[..., :hd], "kv planes": ws[:B * skvp * 4 * hd].view(B, skvp, 4 * hd)[:, :S]}


@pytest.mark.parametrize("ring, bn", [(2, 128), (3, 128), (2, 64)])
def test_h3_gemm_lds_epilogue_and_row_statistics(gemm, ring, bn):
    """MODE 2 (the residual GEMMs of a transformer: C through LDS, the tile held in the ring), N = 1028:
    81 tiles of 128 x 128 (153 of 128 x 64) > 64.  Every epilogue of ``linear``; C and the row statistics
    of ``linear_planes(row_stats=True)``."""
    ops.set_gemm_f32h3_hot_ring(ring)
    ops.set_gemm_f32h3_hot_bn(bn)
    x, (w, b, r, _) = gemm["x"], gemm[1028]
    ap, rinv = ops._split_rows_h3(x, ln=False)
    a = ops.H3Planes(ap, rinv, 0.0, (M, K))

    def run():
        outs = {}
        for act in (None, "gelu", "relu"):
            for res in (None, r):
                outs[f"linear act={act} residual={res is not None}"] = _linear(x, w, b, act, res)
        c, st = _nan32(M, 1028), _nan32(M, -(-1028 // bn), 2)
        ops.linear_planes(a, w, b, residual=r, row_stats=True, out=c, stats_out=st)
        outs["row_stats C"], outs["row_stats statistics"] = c, st
        return outs

    _bit_identical_under_budgets(run, f"MODE 2 ring {ring} bn {bn}")


def test_h3_gemm_register_epilogue(gemm):
    """MODE 0 with fp32 C: N = 1030 (N % 4 != 0 refuses the LDS epilogue) and N = 1028 with the LDS
    epilogue switched off; 81 tiles > 64 both."""
    x = gemm["x"]

    def run():
        outs = {}
        for N, lds in ((1030, True), (1028, False)):
            w, b, r, _ = gemm[N]
            ops.set_gemm_f32h3_lds_epilogue(lds)
            for act, res in ((None, None), ("gelu", r), ("relu", None), (None, r)):
                outs[f"N={N} act={act} residual={res is not None}"] = _linear(x, w, b, act, res)
        ops.set_gemm_f32h3_lds_epilogue(True)
        return outs

    _bit_identical_under_budgets(run, "MODE 0 fp32 C")


def test_h3_gemm_plane_output(gemm):
    """MODE 0 writing the next GEMM's A planes (fc1 -> fc2, GELU; the split pass feeds it): N = 1032
    (ldp % 8 == 0: the LDS-staged 16-byte stores) and N = 1028 (2-byte stores); 81 tiles > 64 both."""
    x = gemm["x"]
    run = lambda: {f"planes N={N}": _ln_to_planes(x, *gemm[N][:2]) for N in (1032, 1028)}
    _bit_identical_under_budgets(run, "MODE 0 planes")


@pytest.mark.parametrize("B", [2, 1])
def test_h3_gemm_kv_plane_output(gemm, B):
    """MODE 0 writing the attention's K / V planes: x [2, 550, 96], 6 heads, N = 1152: 9 x 9 = 81 tiles
    > 64 (two sequences: a tile straddles them, the per-element stores); and one sequence of 1100 (the
    interior tiles through the LDS-staged 16-byte stores).  The Q columns and every plane row of a token."""
    w, b = gemm[1152][:2]
    x3 = gemm["x"].view(B, M // B, K)

    def run():
        qkv, ws, _ = _ln_qkv(x3, w, b, 6)
        return _qkv_outputs(qkv, ws, 6)

    _bit_identical_under_budgets(run, "MODE 0 K/V planes")


@pytest.mark.parametrize("bn", [128, 64])
def test_h3_gemm_layernorm_in_the_a_load(gemm, bn):
    """MODE 1 (``set_ln_handoff(True)``: the LN-GEMM normalises and splits its rows itself), 128 x 128
    tiles, 81 > 64 for every N: fp32 C (N = 1030, 1028), plane output (N = 1032, 1028), K / V output
    (N = 1152), each with the statistics of ``nos_row_stats`` and with ``pre=`` statistics written by a
    row-statistics producer (MODE 2, N = 96: one part of 96 columns at bn 128, parts of 64 + 32 at bn 64;
    the N = 1028 output of the LDS-epilogue case is no legal K, K % 32 == 0)."""
    ops.set_gemm_f32h3_hot_bn(bn)
    ops.set_ln_handoff(True)
    xin, wp, bp, rp = gemm["producer"]
    ap, rinv = ops._split_rows_h3(xin, ln=False)
    a = ops.H3Planes(ap, rinv, 0.0, (M, 64))
    x, st = ops.linear_planes(a, wp, bp, residual=rp, row_stats=True, out=_nan32(M, K),
                              stats_out=_nan32(M, -(-K // bn), 2))
    torch.cuda.synchronize()
    assert st.pw == bn and torch.isfinite(x).all() and torch.isfinite(st.stats).all()

    def run():
        outs = {}
        for name, pre in (("nos_row_stats", None), ("producer statistics", st)):
            for N in (1030, 1028):
                w, b, _, c1 = gemm[N]
                outs[f"{name} C N={N}"] = _linear_ln(x, w, b, c1, "gelu" if N == 1030 else None, pre)
            for N in (1032, 1028):
                outs[f"{name} planes N={N}"] = _ln_to_planes(x, *gemm[N][:2], pre)
            qkv, ws, _ = _ln_qkv(x.view(2, M // 2, K), *gemm[1152][:2], 6, pre)
            for k, v in _qkv_outputs(qkv, ws, 6).items():
                outs[f"{name} qkv {k}"] = v
        return outs

    _bit_identical_under_budgets(run, f"MODE 1 bn {bn}")


def _place(src: torch.Tensor, strides: tuple, fill: float) -> torch.Tensor:
    size = sum((n - 1) * s for n, s in zip(src.shape, strides)) + 1
    buf = torch.full((size,), fill, dtype=src.dtype, device=src.device)
    buf.as_strided(src.shape, strides).copy_(src)
    return buf


def test_h3_gemm_batched_entry_has_no_persistent_form():
    """``nos_gemm_f32h3_batched`` always launches one workgroup per tile (its persistent form spilled):
    the operands of test_gemm_h3_strides_gpu.py::test_batched_strides (nb = 3) under budget 8."""
    nb, m, n, k = 3, 40, 36, 32
    lda, ldw, ldr, ldc = 40, 48, 44, 52
    aplane, wplane = m * lda + 8, n * ldw + 8
    sa, srinv, sw, scsc, sbias, sr, sc = 2 * aplane + 16, m + 3, 2 * wplane + 24, n + 5, m + 7, m * ldr + 9, m * ldc + 11
    g = torch.Generator(device="cuda").manual_seed(12)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, w, bias, res = r(nb, m, k), r(nb, n, k), r(nb, m), r(nb, m, n)
    ap, rinv = zip(*(ops._split_rows_h3(x[b], ln=False) for b in range(nb)))
    wp, csc = zip(*(ops.split_f32_weight_h3(w[b]) for b in range(nb)))
    ap_s = _place(torch.stack(ap), (sa, aplane, lda, 1), math.nan)
    wp_s = _place(torch.stack(wp), (sw, wplane, ldw, 1), math.nan)
    rinv_s, csc_s, bias_s = (_place(t, (s, 1), math.nan)
                             for t, s in ((torch.stack(rinv), srinv), (torch.stack(csc), scsc), (bias, sbias)))
    res_s = _place(res, (sr, ldr, 1), math.nan)

    def run():
        c_s = _nan32((nb - 1) * sc + (m - 1) * ldc + n)
        assert _lib.lib().nos_gemm_f32h3_batched(ap_s.data_ptr(), lda, aplane, sa, rinv_s.data_ptr(), srinv, 0.0,
                                                 wp_s.data_ptr(), ldw, wplane, sw, csc_s.data_ptr(), scsc,
                                                 bias_s.data_ptr(), sbias, res_s.data_ptr(), ldr, sr, c_s.data_ptr(),
                                                 ldc, sc, m, n, k, nb, EPI_BIAS_ROW | EPI_RESID, _stream()) == 0
        return {"C": c_s.as_strided((nb, m, n), (sc, ldc, 1))}

    ref = _under(0, run)
    got = _under(8, run)
    _assert_written(got, "batched budget 8")
    _assert_same_bits(ref, got, "batched budget 8")


# ------------------------------------------------------------------ 2. the head-dim-64 h3 attention
# The planes of the K / V case: B = 2, S = 550, H = 6: 3 query blocks of 256 rows per (batch, head),
# 2 x 6 x 3 = 36 items of 512 threads > 32 (72 under a forced split of 2).
ATT_B, ATT_S, ATT_H = 2, 550, 6


def _attn_h3_planes(qkv, ws, sc, H, osc: float) -> torch.Tensor:
    """``ops.attention_presplit_h3(planes_out=osc)`` into NaN-filled planes."""
    B, S, three_hd = qkv.shape
    hd = three_hd // 3
    planes = _nan16(2, B * S, hd)
    rc = _lib.lib().nos_attn_fwd_f32h3_presplit_d64(qkv.data_ptr(), planes.data_ptr(), B, H, S, S, qkv.stride(1),
                                                    qkv.stride(0), hd, S * hd, 0.125, sc.data_ptr(), ws.data_ptr(),
                                                    ws.numel() * 2, planes.data_ptr(), B * S * hd, osc, _stream())
    assert rc == 0
    return planes


def _poison_partials(ws, B, S, H) -> None:
    """The key-split partials behind the planes of the head-dim-64 workspace."""
    ws[B * ((S + 31) // 32 * 32) * 4 * H * 64:].fill_(-1)


@pytest.mark.parametrize("variant", ["h3n", "h3k2"])
def test_h3_d64_attention(gemm, variant):
    """``attn_fwd_f32h3_d64_kernel<true>``, the YOLOS attention of every pod: 36 items (h3k2: 72) of 512
    threads > 32.  The split is forced, so both runs take the same one: fp32 O and the plane output (the
    merge kernel's PLANES path under h3k2) bit for bit."""
    B, S, H = ATT_B, ATT_S, ATT_H
    ops.set_attention_f32_variant(variant)
    qkv, ws, sc = _ln_qkv(gemm["x"].view(B, S, K), *gemm[1152][:2], H)
    osc = float(sc[1].min())

    def run():
        _poison_partials(ws, B, S, H)
        o = ops.attention_presplit_h3(qkv, ws, sc, H, out=_nan32(B, S, H * 64))
        _poison_partials(ws, B, S, H)
        return {"O": o, "O planes": _attn_h3_planes(qkv, ws, sc, H, osc)}

    _bit_identical_under_budgets(run, variant)


def test_h3_d64_attention_auto_split_under_a_budget(gemm):
    """Variant "h3" picks the split from the CUs it plans for: four on a whole GPU, one at budget 8 (36
    items >= 2 x 8 slots), so the budgeted O is compared with fp64 (LayerNorm, projection and attention)
    at the tolerance of test_attention_h3_gpu.py::test_h3_key_splits_and_tail_tiles."""
    B, S, H = ATT_B, ATT_S, ATT_H
    ops.set_attention_f32_variant("h3")
    w, b = gemm[1152][:2]
    x3 = gemm["x"].view(B, S, K)
    qkv, ws, sc = _ln_qkv(x3, w, b, H)
    o = _under(8, lambda: ops.attention_presplit_h3(qkv, ws, sc, H, out=_nan32(B, S, H * 64)))
    xd = torch.nn.functional.layer_norm(x3.double(), (K,), None, None, EPS)
    q, k, v = (xd @ w.double().t() + b.double()).view(B, S, 3, H, 64).unbind(2)
    p = torch.softmax((q.transpose(1, 2) @ k.transpose(1, 2).transpose(-1, -2)) / 8.0, dim=-1)
    ref = (p @ v.transpose(1, 2)).transpose(1, 2).reshape(B, S, H * 64)
    assert torch.isfinite(o).all()
    err = (o.double() - ref).abs().max().item()
    print(f"h3 auto split at budget 8: max error vs fp64 {err:.3e} (|ref| max {ref.abs().max().item():.3g})")
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), err


# ------------------------------------------------------------------ 3. the general h3 attention forward
# B = 2, Hkv = 2, g = 4 (H = 8), Sq = 600 or 520: 3 query blocks of 256 rows per (batch, head),
# 2 x 8 x 3 = 48 items of 512 threads > 32 (96 under a forced split of 2).
FWD_B, FWD_HKV, FWD_G = 2, 2, 4


def _fwd_inputs(D, sq, skv):
    g = torch.Generator(device="cuda").manual_seed(131 * D + sq + skv)
    return (torch.randn(FWD_B, sq, FWD_HKV * FWD_G, D, device="cuda", generator=g),
            torch.randn(FWD_B, skv, FWD_HKV, D, device="cuda", generator=g),
            torch.randn(FWD_B, skv, FWD_HKV, D, device="cuda", generator=g))


def _rope_tables(S, D):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, device="cuda", dtype=torch.float32) / D))
    ang = torch.arange(S, device="cuda", dtype=torch.float32)[:, None] * inv[None, :]
    ang = torch.cat([ang, ang], 1)
    return ang.cos().contiguous(), ang.sin().contiguous()


def _sdpa_lse_into(q, k, v, causal, workspace):
    """``T.sdpa_lse`` into NaN-filled o and lse (``nos_attn_h3g_lse``)."""
    B, Sq, H, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    o, lse = _nan32(B, Sq, H, D), _nan32(B, H, Sq)
    L = _lib.lib()
    nbytes = int(L.nos_attn_h3g_workspace(B, H, Hkv, Sq, Skv, D))
    ws, wptr = workspace(nbytes, q.device)
    rc = L.nos_attn_h3g_lse(q.data_ptr(), q.stride(1), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0),
                            v.data_ptr(), v.stride(1), v.stride(0), o.data_ptr(), o.stride(1), o.stride(0), B, H, Hkv,
                            Sq, Skv, D, int(causal), 1.0 / math.sqrt(D), None, None, 0.0, wptr, nbytes, lse.data_ptr(),
                            _stream())
    assert rc == 0
    return o, lse


def _rel(a, b, zero_den: float = 1.0) -> float:
    """test_flash_attention_train_gpu.py ``_rel``."""
    den = float(b.double().abs().max())
    return float((a.double() - b.double()).abs().max()) / (den if den > 0 else zero_den)


def _check(names, ours, r64, r32, dens) -> None:
    """test_flash_attention_train_gpu.py ``_check``: rel(ours) <= max(4 rel(torch fp32), 1e-5) against fp64."""
    for name, a, b, c, zd in zip(names, ours, r64, r32, dens):
        assert torch.isfinite(a).all(), name
        ea, ec = _rel(a, b, zd), _rel(c, b, zd)
        print(f"{name}: rel(ours) {ea:.3e}  rel(torch fp32) {ec:.3e}")
        assert ea <= max(4 * ec, 1e-5), (name, ea, ec)


@pytest.mark.parametrize("sq, skv", [(600, 600), (520, 700)])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_h3g_attention_forward(poisoned_workspaces, D, causal, sq, skv):
    """``attn_h3g_kernel<D, CAUSAL, ROPE, true>`` (sdpa, sdpa_lse, decoder prefill): 48 items of 512
    threads > 32.  Under a forced split of 1 and of 2 (96 items, the merge kernel) o and lse equal budget
    0 bit for bit; the causal (600, 600) case also with rotary.  In auto mode the split follows the CUs
    (four on a whole GPU, one at budget 8: 48 items >= the 16 or 8 slots), so the budgeted o is compared
    with fp64 under test_flash_attention_train_gpu.py's ``_check`` and lse under the criterion of its
    test_forward_is_sdpa_bit_for_bit_and_adds_the_log_sum_exp."""
    q, k, v = _fwd_inputs(D, sq, skv)
    rope = _rope_tables(skv, D) if (causal and sq == skv) else None

    def run():
        outs = {}
        outs["sdpa o"] = T.sdpa(q, k, v, causal, out=_nan32(*q.shape))
        outs["sdpa_lse o"], outs["sdpa_lse lse"] = _sdpa_lse_into(q, k, v, causal, poisoned_workspaces)
        if rope is not None:
            outs["sdpa rope o"] = T.sdpa(q, k, v, causal, rope=rope, out=_nan32(*q.shape))
        return outs

    for split in (1, 2):
        T.set_attention_h3g_kvsplit(split)
        ref = _bit_identical_under_budgets(run, f"kvsplit {split}")
        assert torch.equal(ref["sdpa o"], ref["sdpa_lse o"])
    T.set_attention_h3g_kvsplit(0)
    got = _under(8, run)
    _assert_written(got, "auto split budget 8")
    q64, k64, v64 = q.double(), k.double(), v.double()
    o64, l64 = T.sdpa_lse_ref(q64, k64, v64, causal)
    o32, l32 = T.sdpa_lse_ref(q, k, v, causal)
    _check(("sdpa o", "sdpa_lse o"), (got["sdpa o"], got["sdpa_lse o"]), (o64, o64), (o32, o32), (1.0, 1.0))
    err, err32 = float((got["sdpa_lse lse"].double() - l64).abs().max()), float((l32.double() - l64).abs().max())
    print(f"lse err {err:.3e}  torch fp32 {err32:.3e}")
    assert err <= max(4 * err32, 1e-5), (err, err32)
    if rope is not None:
        _check(("sdpa rope o",), (got["sdpa rope o"],), (T.sdpa_ref(q64, k64, v64, causal, rope=rope),),
               (T.sdpa_ref(q, k, v, causal, rope=rope),), (1.0,))


# ------------------------------------------------------------------ 4. the flash-attention backward
# B = 3, Hkv = 4, g = 2 (H = 8), Sq = Skv = 700, 256 threads per workgroup (at most 64 at budget 8):
#   dK / dV: 6 key blocks of 128 per (batch, kv head): 3 x 4 x 6 = 72 items > 64
#   dQ:      6 query blocks of 128 per (batch, head):  3 x 8 x 6 = 144 items > 64
# One range of the query sweep under both budgets (72 items >= 8 and >= 20 CUs); three on a whole GPU.
BWD_B, BWD_HKV, BWD_G, BWD_S = 3, 4, 2, 700


def _ref_attention(q, k, v, causal):
    """test_flash_attention_train_gpu.py ``_ref``."""
    g = q.shape[2] // k.shape[2]
    k, v = k.repeat_interleave(g, 2), v.repeat_interleave(g, 2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / q.shape[-1] ** 0.5
    if causal:
        i = torch.arange(q.shape[1], device=q.device)[:, None] + (k.shape[1] - q.shape[1])
        s = s.masked_fill(torch.arange(k.shape[1], device=q.device)[None, :] > i, float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v)


def _autograd(q, k, v, do, causal):
    xs = [x.detach().clone().requires_grad_(True) for x in (q, k, v)]
    y = _ref_attention(*xs, causal)
    y.backward(do.to(y.dtype))
    return [x.grad for x in xs]


def _zero_dens(q, k, v, do):
    """test_flash_attention_train_gpu.py ``_zero_dens`` for (dq, dk, dv)."""
    g = q.shape[2] // k.shape[2]
    dp = torch.einsum("bqhd,bkhd->bhqk", do.double(), v.double().repeat_interleave(g, 2)).abs().max()
    sc = q.shape[-1] ** -0.5
    return [float(sc * dp * k.abs().max()), float(sc * dp * q.abs().max()), 1.0]


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_h3g_attention_backward(poisoned_workspaces, D, causal):
    """``attn_h3g_bwd_dkdv_kernel`` (72 items > 64) and ``attn_h3g_bwd_dq_kernel`` (144 > 64).  dq, dk, dv
    are bit-equal between budgets 8 and 20 (one sweep range under both); dq also to budget 0 (the dQ
    kernel takes no split).  On a whole GPU dk and dv run three sweep ranges, so the budgeted gradients
    are compared with fp64 autograd under test_flash_attention_train_gpu.py's ``_check`` and ``_zero_dens``."""
    gen = torch.Generator(device="cuda").manual_seed(7 * D + causal)
    H = BWD_HKV * BWD_G
    q, do = (torch.randn(BWD_B, BWD_S, H, D, device="cuda", generator=gen) for _ in range(2))
    k, v = (torch.randn(BWD_B, BWD_S, BWD_HKV, D, device="cuda", generator=gen) for _ in range(2))
    o, lse = T.sdpa_lse(q, k, v, causal)

    def run():
        out = tuple(torch.full_like(t, math.nan) for t in (q, k, v))
        T.sdpa_bwd(q, k, v, o, lse, do, causal, out=out)
        return dict(zip(("dq", "dk", "dv"), out))

    g0, g8, g20 = (_under(budget, run) for budget in (0, 8, 20))
    for budget, g in ((0, g0), (8, g8), (20, g20)):
        _assert_written(g, f"budget {budget}")
    _assert_same_bits(g8, g20, "budget 20 against budget 8:")
    _assert_same_bits({"dq": g0["dq"]}, {"dq": g8["dq"]}, "budget 8 against budget 0:")
    r64 = _autograd(q.double(), k.double(), v.double(), do.double(), causal)
    r32 = _autograd(q, k, v, do, causal)
    _check(("dq", "dk", "dv"), (g8["dq"], g8["dk"], g8["dv"]), r64, r32, _zero_dens(q, k, v, do))


# ------------------------------------------------------------------ 5. int8
def _q8_weights(N: int, Kq: int, seed: int):
    """test_linear_q8_gpu.py ``_weights``: full-range int8 rows, an all-zero row, a zero scale."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-128, 128, (N, Kq), generator=g, dtype=torch.int32).to(torch.int8)
    sc = (torch.rand(N, generator=g) + 0.5) / (64.0 * Kq ** 0.5)
    q[0, 0], q[0, Kq - 1] = -128, 127
    q[1] = 0
    sc[2] = 0.0
    return q.cuda(), sc.cuda()


@pytest.mark.parametrize("Mq", [1, 8])
def test_gemv_q8_walks_its_column_groups_under_a_budget(Mq):
    """``gemv_q8_kernel``: N = 1000, K = 1024.  Plain epilogue: 63 groups of 16 columns (the last one 8
    wide); GLU: 63 groups of 8 gate / up pairs (the last one 4).  The grid is 3 workgroups per CU: at
    most 24 at budget 8 (three trips, the next group's weights prefetched), 60 at budget 20 (two trips
    for three of them).  No output's summation order depends on the grid."""
    N, Kq = 1000, 1024
    torch.manual_seed(Mq)
    q, sc = _q8_weights(N, Kq, Mq)
    x = torch.randn(Mq, Kq, device="cuda")
    gamma = 1 + 0.1 * torch.randn(Kq, device="cuda")
    b, r = torch.randn(N, device="cuda"), torch.randn(Mq, N, device="cuda")
    assert T.gemv_q8_ok(x, q)

    def into(y, bias, res, act, rms_eps, glu):
        rc = _lib.lib().nos_gemv_q8(x.data_ptr(), x.stride(0), q.data_ptr(), q.stride(0), sc.data_ptr(),
                                    gamma.data_ptr() if rms_eps else None, None if bias is None else bias.data_ptr(),
                                    None if res is None else res.data_ptr(), 0 if res is None else res.stride(0),
                                    y.data_ptr(), y.stride(0), Mq, N, Kq, T._q8_epi(bias, act, res, glu), rms_eps,
                                    _stream())
        assert rc == 0
        return y

    def run():
        return {"plain": into(_nan32(Mq, N), None, None, None, 0.0, False),
                "bias gelu residual rms": into(_nan32(Mq, N), b, r, "gelu", 1e-5, False),
                "glu": into(_nan32(Mq, N // 2), None, None, None, 0.0, True),
                "glu bias rms": into(_nan32(Mq, N // 2), b, None, None, 1e-5, True)}

    ref = _bit_identical_under_budgets(run, "gemv_q8")
    assert torch.equal(ref["bias gelu residual rms"], T.gemv_q8(x, q, sc, b, "gelu", r, rms_eps=1e-5, gamma=gamma))
    assert torch.equal(ref["glu"], T.gemv_q8(x, q, sc, glu=True))


def test_dequant_q8_stride_loop_under_a_budget():
    """``nos_dequant_q8``: N = 1000, K = 1024 is 1000 blocks of 256 threads over a cap of 32 x 8 = 256
    (four trips of the grid-stride loop, the last one 232 blocks) and of 32 x 20 = 640 (two trips);
    test_linear_q8_gpu.py::test_dequant_q8_is_bit_exact's reference."""
    N, Kq = 1000, 1024
    q, sc = _q8_weights(N, Kq, N)

    def run():
        out = _nan32(N, Kq)
        assert _lib.lib().nos_dequant_q8(q.data_ptr(), q.stride(0), sc.data_ptr(), out.data_ptr(), Kq, N, Kq,
                                         _stream()) == 0
        return {"dequantized": out}

    ref = _bit_identical_under_budgets(run, "dequant_q8")
    assert torch.equal(ref["dequantized"], q.float() * sc[:, None])


# ------------------------------------------------------------------ 6. a slice pod end to end
def test_yolos_program_under_a_slice_pods_configuration():
    """The YOLOS-small demo program of test_ln_handoff_gpu.py::test_yolos_program_with_and_without_the_handoff
    (h3 math, "h3n", hand-off on) compiled and run at budgets 0 and 32, under that test's bound for two
    schedules of the same arithmetic.  The outputs are in fact bit-equal: with the key split forced to
    one, no op of the program depends on the budget."""
    from nos_amd.models.yolos_program import demo_tenant
    from nos_amd.podserver import program as PG

    prog, w = demo_tenant("fp32", 0, small=True)
    p = PG.parse(prog, w, gpu=True)
    x = p.input_tensor("cuda", torch.randn(p.inputs[0].shape, generator=torch.Generator().manual_seed(0)).numpy())
    ops.set_attention_f32_variant("h3n")
    ops.set_ln_handoff(True)

    def run():
        cm = p.compile("cuda")
        with torch.no_grad():
            return [o.clone() for o in cm(x)]

    t0 = time.perf_counter()
    a, b = _under(0, run), _under(32, run)
    assert len(a) == len(b) > 0
    same = all(torch.equal(u, v) for u, v in zip(a, b))
    print(f"YOLOS-small at budgets 0 and 32: outputs bit-equal: {same} ({time.perf_counter() - t0:.2f} s)")
    for u, v in zip(a, b):
        assert torch.isfinite(v).all()
        assert ((u - v).abs().max() / u.abs().max()) <= 1e-5
