"""The four ``nos_gemm_f32h3*`` entry points with every leading dimension,
plane stride and batch stride distinct and larger than its extent, bit for bit
against the same call on contiguous copies.  A tile's arithmetic does not
depend on the strides, and every stride keeps the alignment that selects the
kernel (lda, ldw % 8; ldx, ldr, ldc % 4), so both calls run the same
instantiation: any difference is an operand read or written through the wrong
stride.  The padding between rows holds NaN (inputs) or a sentinel (outputs)."""
from __future__ import annotations

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

EPI_BIAS, EPI_GELU, EPI_RESID, EPI_BIAS_ROW = 1, 2, 4, 16
M, N, K = 130, 132, 64  # two row tiles and two column tiles, each with a tail; two K stages
LDA, LDW, LDR, LDC, LDX = 72, 80, 136, 140, 68
SENTINEL = -777.0


def _place(src: torch.Tensor, strides: tuple, fill: float) -> torch.Tensor:
    """src copied into a fresh flat buffer at the given element strides, `fill` everywhere else."""
    size = sum((n - 1) * s for n, s in zip(src.shape, strides)) + 1
    buf = torch.full((size,), fill, dtype=src.dtype, device=src.device)
    buf.as_strided(src.shape, strides).copy_(src)
    return buf


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def L():
    from nos_amd.ops import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def ops_():
    from nos_amd import ops

    return ops


@pytest.fixture(scope="module")
def data(ops_):
    g = torch.Generator(device="cuda").manual_seed(11)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, w, bias, res = r(M, K), r(N, K), r(N), r(M, N)
    ap, rinv = ops_._split_rows_h3(x, ln=False)
    wp, csc = ops_.split_f32_weight_h3(w)
    torch.cuda.synchronize()
    return dict(x=x, ap=ap, rinv=rinv, wp=wp, csc=csc, bias=bias, res=res,
                ap_s=_place(ap, (M * LDA + 8, LDA, 1), math.nan), wp_s=_place(wp, (N * LDW + 16, LDW, 1), math.nan),
                res_s=_place(res, (LDR, 1), math.nan), x_s=_place(x, (LDX, 1), math.nan))


def _out(ld: int, rows: int = M) -> torch.Tensor:
    return torch.full((rows, ld), SENTINEL, device="cuda")


def _check_c(c_s: torch.Tensor, c: torch.Tensor) -> None:
    torch.cuda.synchronize()
    assert torch.isfinite(c).all()
    assert _same_bits(c_s[:, :c.shape[1]], c)
    assert (c_s[:, c.shape[1]:] == SENTINEL).all(), "nothing is written between the rows of C"


def test_gemm_strides(L, ops_, data):
    d, st, epi = data, ops_._stream(), EPI_BIAS | EPI_GELU | EPI_RESID
    c, c_s = _out(N), _out(LDC)
    tail = (epi, None, 0, 0, None, None, 0, 0, 1.0, st)
    assert L.nos_gemm_f32h3(d["ap"].data_ptr(), K, M * K, d["rinv"].data_ptr(), 0.0, d["wp"].data_ptr(), K, N * K,
                            d["csc"].data_ptr(), d["bias"].data_ptr(), d["res"].data_ptr(), N, c.data_ptr(), N, M, N,
                            K, *tail) == 0
    assert L.nos_gemm_f32h3(d["ap_s"].data_ptr(), LDA, M * LDA + 8, d["rinv"].data_ptr(), 0.0, d["wp_s"].data_ptr(),
                            LDW, N * LDW + 16, d["csc"].data_ptr(), d["bias"].data_ptr(), d["res_s"].data_ptr(), LDR,
                            c_s.data_ptr(), LDC, M, N, K, *tail) == 0
    _check_c(c_s, c)


def test_gemm_plane_output_strides(L, ops_, data):
    """The output as the next GEMM's A planes: ldp and pplane."""
    d, st, ldp = data, ops_._stream(), 144
    pplane = M * ldp + 24
    p = torch.full((2, M, N), SENTINEL, dtype=torch.float16, device="cuda")
    p_s = torch.full((2 * pplane,), SENTINEL, dtype=torch.float16, device="cuda")
    head = (d["rinv"].data_ptr(), 0.0)
    assert L.nos_gemm_f32h3(d["ap"].data_ptr(), K, M * K, *head, d["wp"].data_ptr(), K, N * K, d["csc"].data_ptr(),
                            d["bias"].data_ptr(), None, 0, None, 0, M, N, K, EPI_BIAS | EPI_GELU, None, 0, 0, None,
                            p.data_ptr(), N, M * N, 0.125, st) == 0
    assert L.nos_gemm_f32h3(d["ap_s"].data_ptr(), LDA, M * LDA + 8, *head, d["wp_s"].data_ptr(), LDW, N * LDW + 16,
                            d["csc"].data_ptr(), d["bias"].data_ptr(), None, 0, None, 0, M, N, K, EPI_BIAS | EPI_GELU,
                            None, 0, 0, None, p_s.data_ptr(), ldp, pplane, 0.125, st) == 0
    torch.cuda.synchronize()
    got = p_s.as_strided((2, M, N), (pplane, ldp, 1))
    assert torch.equal(got.contiguous().view(torch.int16), p.view(torch.int16))
    untouched = p_s.clone()
    untouched.as_strided((2, M, N), (pplane, ldp, 1)).fill_(SENTINEL)
    assert (untouched == SENTINEL).all(), "nothing is written between the rows of the planes"


def test_stats_strides(L, ops_, data):
    d, st, epi = data, ops_._stream(), EPI_BIAS | EPI_RESID
    parts = -(-N // ops_.stats_pw())
    c, c_s = _out(N), _out(LDC)
    s, s_s = torch.zeros(M, parts, 2, device="cuda"), torch.zeros(M, parts, 2, device="cuda")
    assert L.nos_gemm_f32h3_stats(d["ap"].data_ptr(), K, M * K, d["rinv"].data_ptr(), 0.0, d["wp"].data_ptr(), K,
                                  N * K, d["csc"].data_ptr(), d["bias"].data_ptr(), d["res"].data_ptr(), N,
                                  c.data_ptr(), N, M, N, K, epi, s.data_ptr(), st) == 0
    assert L.nos_gemm_f32h3_stats(d["ap_s"].data_ptr(), LDA, M * LDA + 8, d["rinv"].data_ptr(), 0.0,
                                  d["wp_s"].data_ptr(), LDW, N * LDW + 16, d["csc"].data_ptr(), d["bias"].data_ptr(),
                                  d["res_s"].data_ptr(), LDR, c_s.data_ptr(), LDC, M, N, K, epi, s_s.data_ptr(),
                                  st) == 0
    _check_c(c_s, c)
    assert _same_bits(s_s, s)


def test_lna_strides(L, ops_, data):
    d, st, epi = data, ops_._stream(), EPI_BIAS | EPI_RESID
    stats = ops_._row_stats(d["x"]).stats  # one part of K columns
    eln = 14 - math.frexp(math.sqrt(K))[1]
    c, c_s = _out(N), _out(LDC)
    mid = (stats.data_ptr(), 1, K, 1e-6, eln)
    tail = (epi, None, 0, 0, None, None, 0, 0, 1.0, st)
    assert L.nos_gemm_f32h3_lna(d["x"].data_ptr(), K, *mid, d["wp"].data_ptr(), K, N * K, d["csc"].data_ptr(),
                                d["bias"].data_ptr(), d["res"].data_ptr(), N, c.data_ptr(), N, M, N, K, *tail) == 0
    assert L.nos_gemm_f32h3_lna(d["x_s"].data_ptr(), LDX, *mid, d["wp_s"].data_ptr(), LDW, N * LDW + 16,
                                d["csc"].data_ptr(), d["bias"].data_ptr(), d["res_s"].data_ptr(), LDR, c_s.data_ptr(),
                                LDC, M, N, K, *tail) == 0
    _check_c(c_s, c)


def test_batched_strides(L, ops_):
    """nb = 3 with seven different batch strides and the bias per row, against three nb = 1 calls on contiguous copies."""
    nb, m, n, k = 3, 40, 36, 32
    lda, ldw, ldr, ldc = 40, 48, 44, 52
    aplane, wplane = m * lda + 8, n * ldw + 8
    sa, srinv, sw, scsc, sbias, sr, sc = 2 * aplane + 16, m + 3, 2 * wplane + 24, n + 5, m + 7, m * ldr + 9, m * ldc + 11
    g = torch.Generator(device="cuda").manual_seed(12)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, w, bias, res = r(nb, m, k), r(nb, n, k), r(nb, m), r(nb, m, n)
    ap, rinv = zip(*(ops_._split_rows_h3(x[b], ln=False) for b in range(nb)))
    wp, csc = zip(*(ops_.split_f32_weight_h3(w[b]) for b in range(nb)))
    ap, rinv, wp, csc = torch.stack(ap), torch.stack(rinv), torch.stack(wp), torch.stack(csc)
    st, epi = ops_._stream(), EPI_BIAS_ROW | EPI_RESID
    want = torch.full((nb, m, n), SENTINEL, device="cuda")
    for b in range(nb):
        assert L.nos_gemm_f32h3_batched(ap[b].data_ptr(), k, m * k, 0, rinv[b].data_ptr(), 0, 0.0, wp[b].data_ptr(), k,
                                        n * k, 0, csc[b].data_ptr(), 0, bias[b].data_ptr(), 0, res[b].data_ptr(), n, 0,
                                        want[b].data_ptr(), n, 0, m, n, k, 1, epi, st) == 0
    ap_s, wp_s = _place(ap, (sa, aplane, lda, 1), math.nan), _place(wp, (sw, wplane, ldw, 1), math.nan)
    rinv_s, csc_s, bias_s = (_place(t, (s, 1), math.nan) for t, s in ((rinv, srinv), (csc, scsc), (bias, sbias)))
    res_s = _place(res, (sr, ldr, 1), math.nan)
    c_s = torch.full(((nb - 1) * sc + (m - 1) * ldc + n,), SENTINEL, device="cuda")
    assert L.nos_gemm_f32h3_batched(ap_s.data_ptr(), lda, aplane, sa, rinv_s.data_ptr(), srinv, 0.0, wp_s.data_ptr(),
                                    ldw, wplane, sw, csc_s.data_ptr(), scsc, bias_s.data_ptr(), sbias,
                                    res_s.data_ptr(), ldr, sr, c_s.data_ptr(), ldc, sc, m, n, k, nb, epi, st) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    assert _same_bits(c_s.as_strided((nb, m, n), (sc, ldc, 1)), want)
    c_s.as_strided((nb, m, n), (sc, ldc, 1)).fill_(SENTINEL)
    assert (c_s == SENTINEL).all(), "nothing is written between the rows and batch elements of C"
