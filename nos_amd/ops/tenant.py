"""Ops of general pod-server tenant programs (decoder LLMs, conv nets).

The YOLOS-class encoder ops live in :mod:`nos_amd.ops`; this module adds
what conv nets and decoder LLMs need, each lowered onto gfx950 kernels of
``libnos_hip.so`` for CUDA tensors and onto a plain PyTorch fp32 reference
for CPU tensors (the numerics tests compare the two):

* :func:`conv2d` -- implicit-GEMM convolution on the fp16x3 (h3) matrix
  pipes: ``nos_im2col_h3`` writes an image's patches straight as the GEMM's
  split planes (per-patch power-of-two scales), and ONE batched
  ``nos_gemm_f32h3_batched`` launch computes ``W . patches^T`` for every
  image, NCHW out, bias per output channel, ReLU / GELU and a residual in
  the epilogue (BatchNorm is folded into the weights by the compiler);
* :func:`matmul` -- batched activation x activation GEMM on the same kernel
  (both sides split at run time, a broadcast side has stride 0);
* :func:`sdpa` -- attention with causal masking, head_dim 64 / 128,
  grouped-query K/V heads and fused rotary embeddings (``nos_attn_h3g``);
* :func:`linear_rms` -- RMSNorm folded into the following GEMM (the row
  statistics in the split pre-pass, gamma in the weight);
* :func:`embedding`, :func:`rmsnorm`, :func:`softmax`, :func:`rotary` --
  row / gather kernels (``tenant_ops.hip``), fp32 and bf16.

bf16 tensors run the fp32-only GEMM / attention kernels on an fp32 copy
(more precision than the tenant asked for, never less).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from . import EPI_BIAS, EPI_GELU, EPI_RELU, EPI_RESID, _lib, _split_rows_h3, _stream, split_f32_weight_h3

EPI_BIAS_ROW, EPI_RESID_PRE = 16, 32  # csrc/hip/epilogue.h; gemm_f32h.hip: bias per row; residual added before the activation


def _ptr(t):
    return None if t is None else t.data_ptr()


def _act_epi(act: str | None) -> int:
    return EPI_GELU if act == "gelu" else (EPI_RELU if act == "relu" else 0)


def _act(y: torch.Tensor, act: str | None) -> torch.Tensor:
    return F.gelu(y) if act == "gelu" else (F.relu(y) if act == "relu" else y)


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype == torch.float32 else t.float()


def _pad_k(t: torch.Tensor, mult: int = 32) -> torch.Tensor:
    k = t.shape[-1]
    kp = -(-k // mult) * mult
    return t if kp == k else F.pad(t, (0, kp - k))


def _bf(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return 1
    if t.dtype == torch.float32:
        return 0
    raise ValueError(f"tenant ops take fp32 or bf16 tensors, got {t.dtype}")


# ------------------------------------------------------------------ references
def _ref_dtype(t: torch.Tensor) -> torch.dtype:
    """The dtype a reference computes in: fp32, or fp64 for fp64 inputs (a
    test's high-precision reference must not be rounded to fp32 on the way)."""
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def conv2d_ref(x, w, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), act=None, residual=None,
               residual_first: bool = False, groups: int = 1):
    y = F.conv2d(x.float(), w.float(), None if bias is None else bias.float(), stride, padding, dilation, groups)
    if residual is not None and residual_first:
        y = y + residual.float()
    y = _act(y, act)
    if residual is not None and not residual_first:
        y = y + residual.float()
    return y.to(x.dtype)


def rope_ref(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos0: int = 0) -> torch.Tensor:
    """rotate_half rotary on x [B, S, H, D] with tables [>= pos0 + S, D]."""
    S, D = x.shape[1], x.shape[-1]
    ct = _ref_dtype(x)
    c = cos[pos0:pos0 + S].to(ct)[None, :, None, :]
    s = sin[pos0:pos0 + S].to(ct)[None, :, None, :]
    xf = x.to(ct)
    rot = torch.cat([-xf[..., D // 2:], xf[..., :D // 2]], dim=-1)
    return (xf * c + rot * s).to(x.dtype)


def sdpa_ref(q, k, v, causal: bool = False, scale: float | None = None, rope=None) -> torch.Tensor:
    """q [B, Sq, H, D], k / v [B, Skv, Hkv, D] -> [B, Sq, H, D] in fp32 math (fp64 inputs: fp64 math)."""
    B, Sq, H, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    ct = _ref_dtype(q)
    qf, kf, vf = q.to(ct), k.to(ct), v.to(ct)
    if rope is not None:
        cos, sin = rope[0], rope[1]
        qf = rope_ref(qf, cos, sin, Skv - Sq)
        kf = rope_ref(kf, cos, sin, 0)
    if Hkv != H:
        kf = kf.repeat_interleave(H // Hkv, dim=2)
        vf = vf.repeat_interleave(H // Hkv, dim=2)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    s = torch.einsum("bqhd,bkhd->bhqk", qf, kf) * scale
    if causal:
        i = torch.arange(Sq, device=q.device)[:, None] + (Skv - Sq)
        j = torch.arange(Skv, device=q.device)[None, :]
        s = s.masked_fill(j > i, float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhqk,bkhd->bqhd", p, vf).to(q.dtype)


def _train_scores(q, k, causal: bool, scale: float):
    """scale q k^T [B, H, Sq, Skv] in q's dtype (grouped-query heads repeated), masked keys at -inf."""
    Sq, Skv = q.shape[1], k.shape[1]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k.repeat_interleave(q.shape[2] // k.shape[2], dim=2)) * scale
    if causal:
        i = torch.arange(Sq, device=q.device)[:, None] + (Skv - Sq)
        j = torch.arange(Skv, device=q.device)[None, :]
        s = s.masked_fill(j > i, float("-inf"))
    return s


def sdpa_lse_ref(q, k, v, causal: bool = False, scale: float | None = None):
    """(o, lse) of :func:`sdpa_lse` in plain torch math in the input dtype
    (fp64 stays fp64): lse [B, H, Sq] = log sum_j exp(scale q_i . k_j) over
    the keys row i sees, o = exp(s - lse) v."""
    ct = _ref_dtype(q)
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    qf, kf, vf = q.to(ct), k.to(ct), v.to(ct)
    s = _train_scores(qf, kf, causal, scale)
    m = s.amax(-1, keepdim=True)
    lse = (m + torch.log(torch.exp(s - m).sum(-1, keepdim=True))).squeeze(-1)
    p = torch.exp(s - lse[..., None])
    o = torch.einsum("bhqk,bkhd->bqhd", p, vf.repeat_interleave(q.shape[2] // k.shape[2], dim=2))
    return o.to(q.dtype), lse


def sdpa_bwd_ref(q, k, v, o, lse, do, causal: bool = False, scale: float | None = None):
    """(dq, dk, dv) of :func:`sdpa_bwd` by the recompute-from-log-sum-exp
    formulas the kernel implements (no autograd): P = exp(s - lse),
    dV = P^T dO, dP = dO V^T, delta = rowsum(dO . O), dS = scale P (dP - delta),
    dQ = dS K, dK = dS^T Q; the heads of a group sum into their K / V head."""
    ct = _ref_dtype(q)
    B, Sq, H, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    g = H // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    qf, kf, vf, of, dof = (t.to(ct) for t in (q, k, v, o, do))
    p = torch.exp(_train_scores(qf, kf, causal, scale) - lse.to(ct)[..., None])
    dp = torch.einsum("bqhd,bkhd->bhqk", dof, vf.repeat_interleave(g, dim=2))
    delta = (dof * of).sum(-1).permute(0, 2, 1)                        # [B, H, Sq]
    ds = p * (dp - delta[..., None]) * scale
    dq = torch.einsum("bhqk,bkhd->bqhd", ds, kf.repeat_interleave(g, dim=2))
    dk = torch.einsum("bhqk,bqhd->bkhd", ds, qf).reshape(B, Skv, Hkv, g, D).sum(3)
    dv = torch.einsum("bhqk,bqhd->bkhd", p, dof).reshape(B, Skv, Hkv, g, D).sum(3)
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


def rmsnorm_ref(x, weight, eps=1e-6):
    ct = _ref_dtype(x)
    xf = x.to(ct)
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (weight.to(ct) * y.to(x.dtype).to(ct)).to(x.dtype)


def linear_rms_ref(x, wg, bias=None, act=None, eps=1e-6):
    ct = _ref_dtype(x)
    xf = x.to(ct)
    y = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)) @ wg.to(ct).t()
    if bias is not None:
        y = y + bias.to(ct)
    return _act(y, act).to(x.dtype)


# ------------------------------------------------------------------ gather / row kernels
def embedding(ids: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """table[ids] for int ids of any shape; out [*ids.shape, D]."""
    if not table.is_cuda:
        return F.embedding(ids.long(), table)
    V, D = table.shape
    ids32 = ids.to(torch.int32).contiguous()
    out = torch.empty((*ids.shape, D), dtype=table.dtype, device=table.device)
    row_bytes = D * table.element_size()
    if row_bytes % 16 or not table.is_contiguous():
        raise ValueError("native embedding needs a contiguous table with 16-byte rows")
    _lib.check(_lib.lib().nos_embedding(ids32.data_ptr(), table.data_ptr(), out.data_ptr(), ids32.numel(), V,
                                        row_bytes, _stream()), "nos_embedding")
    return out


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    if not x.is_cuda:
        return rmsnorm_ref(x, weight, eps)
    D = x.shape[-1]
    x2 = x.reshape(-1, D)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    w = weight.to(x.dtype).contiguous()
    out = torch.empty(x2.shape, dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().nos_rmsnorm(x2.data_ptr(), w.data_ptr(), out.data_ptr(), x2.shape[0], D, x2.stride(0), D,
                                      float(eps), _bf(x), _stream()), "nos_rmsnorm")
    return out.view(x.shape)


UNARY_CODES = {"relu": 1, "sigmoid": 2, "silu": 3, "gelu": 4, "tanh": 5, "exp": 6, "neg": 7}


def unary(x: torch.Tensor, op: str, dtype: torch.dtype) -> torch.Tensor:
    """``op`` (a :data:`UNARY_CODES` activation) of fp32 / bf16 x into a
    ``dtype`` tensor: evaluated in fp32 and rounded once, in one pass on the
    GPU (a cast beside an activation costs no launch of its own)."""
    if not x.is_cuda:
        xf = x.float()
        y = {"relu": F.relu, "sigmoid": torch.sigmoid, "silu": F.silu, "gelu": F.gelu, "tanh": torch.tanh,
             "exp": torch.exp, "neg": torch.neg}[op](xf)
        return y.to(dtype)
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    if not out.numel():
        return out
    N = x.shape[-1] if x.dim() else 1
    try:   # rows at a uniform stride (e.g. a column slice of a merged GEMM's output): read in place
        x2 = x.view(-1, N) if x.dim() > 1 else None
    except RuntimeError:
        x2 = None
    if x2 is not None and not x.is_contiguous() and x2.stride(-1) == 1:
        _lib.check(_lib.lib().nos_unary_rows(x2.data_ptr(), x2.stride(0), _bf(x2), out.data_ptr(),
                                             int(dtype == torch.bfloat16), x2.shape[0], N, UNARY_CODES[op], _stream()),
                   "nos_unary_rows")
        return out
    xc = x.contiguous()
    _lib.check(_lib.lib().nos_unary(xc.data_ptr(), _bf(xc), out.data_ptr(), int(dtype == torch.bfloat16),
                                    xc.numel(), UNARY_CODES[op], _stream()), "nos_unary")
    return out


def glu(a: torch.Tensor, b: torch.Tensor, op: str = "silu") -> torch.Tensor:
    """f(a) * b in one pass (SwiGLU: silu(gate) * up), a and b of one shape
    and dtype; rows of a and b may be strided (column slices of one GEMM)."""
    f = {"relu": F.relu, "sigmoid": torch.sigmoid, "silu": F.silu, "gelu": F.gelu}[op]
    if not a.is_cuda or a.shape != b.shape or a.dtype != b.dtype or a.dtype not in (torch.float32, torch.bfloat16):
        return (f(a.float()) * b.float()).to(a.dtype)
    N = a.shape[-1]

    def rows(t):
        t2 = t.reshape(-1, N) if t.is_contiguous() else None
        if t2 is None:
            try:
                t2 = t.view(-1, N)
            except RuntimeError:
                t2 = t.contiguous().view(-1, N)
        return t2 if t2.stride(-1) == 1 else t2.contiguous()

    a2, b2 = rows(a), rows(b)
    out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    if out.numel():
        _lib.check(_lib.lib().nos_glu(a2.data_ptr(), a2.stride(0), b2.data_ptr(), b2.stride(0), out.data_ptr(),
                                      a2.shape[0], N, UNARY_CODES[op], _bf(a), _stream()), "nos_glu")
    return out


def softmax(x: torch.Tensor) -> torch.Tensor:
    """softmax over the last dim."""
    if not x.is_cuda:
        return torch.softmax(x.float(), dim=-1).to(x.dtype)
    L = x.shape[-1]
    x2 = x.reshape(-1, L)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    out = torch.empty(x2.shape, dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().nos_softmax(x2.data_ptr(), out.data_ptr(), x2.shape[0], L, x2.stride(0), L, _bf(x),
                                      _stream()), "nos_softmax")
    return out.view(x.shape)


def _rows(x: torch.Tensor, aligned: bool = False) -> tuple[torch.Tensor, int, int]:
    """x [B, S, H, D] as the kernels take it: (x or a copy, token row stride,
    batch stride), copied only when its heads are not contiguous per token
    (a slice of a fused projection is taken as it is).  ``aligned`` (the h3
    attention): in fp32, and also copied when a stride is no multiple of 4
    floats or the pointer not 16-byte aligned."""
    if aligned:
        x = _f32(x)
    if x.stride(-1) != 1 or x.stride(-2) != x.shape[-1]:
        x = x.contiguous()
    if aligned and (x.stride(1) % 4 or x.stride(0) % 4 or x.data_ptr() % 16):
        x = x.clone(memory_format=torch.contiguous_format)
    return x, x.stride(1), x.stride(0)


def _workspace(nbytes: int, device) -> tuple[torch.Tensor, int]:
    """nbytes of device scratch: (the tensor that owns it, its 256-byte aligned pointer)."""
    ws = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
    return ws, (ws.data_ptr() + 255) // 256 * 256


def rotary(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """rotate_half rotary embedding of x [B, S, H, D] with fp32 tables [S, D]."""
    if not x.is_cuda:
        return rope_ref(x, cos, sin)
    B, S, H, D = x.shape
    x, ld, bs = _rows(x)
    c, s = cos.float().contiguous(), sin.float().contiguous()
    if c.shape[0] < S or c.shape[1] != D:
        raise ValueError(f"rotary tables must be [>= {S}, {D}]")
    out = torch.empty((B, S, H, D), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().nos_rotary(x.data_ptr(), c.data_ptr(), s.data_ptr(), out.data_ptr(), B, S, H, D, ld, bs,
                                     _bf(x), _stream()), "nos_rotary")
    return out


# ------------------------------------------------------------------ GEMM-class ops (h3)
def _gemm_batched(ap, rinv, sa, srinv, wp, csc, sw, scsc, out, M, N, K, nb, epi, bias=None, residual=None,
                  ldc=None, sc=None, ldr=None, sr=None, sbias=0, c_off=0, w_off=0, wr_off=0) -> None:
    """``c_off`` / ``w_off`` / ``wr_off``: element offsets of batch element
    0's C, W-operand planes and W-operand row scales (a grouped conv's image
    n; the planes keep the whole tensor's plane stride)."""
    L = _lib.lib()
    ldc = N if ldc is None else ldc
    rc = L.nos_gemm_f32h3_batched(ap.data_ptr(), K, ap[0].numel(), sa,
                                  rinv.data_ptr(), srinv, 0.0, wp.data_ptr() + 2 * w_off, K, wp[0].numel(), sw,
                                  csc.data_ptr() + 4 * wr_off, scsc, _ptr(bias), sbias, _ptr(residual), ldr or ldc,
                                  sr or 0, out.data_ptr() + 4 * c_off, ldc, M * ldc if sc is None else sc, M, N, K, nb,
                                  epi, _stream())
    _lib.check(rc, "nos_gemm_f32h3_batched")


def conv2d(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, stride=(1, 1), padding=(0, 0),
           dilation=(1, 1), act: str | None = None, residual: torch.Tensor | None = None,
           w2: torch.Tensor | None = None, residual_first: bool = False, groups: int = 1) -> torch.Tensor:
    """act(conv2d(x, w) + bias) + residual, NCHW
    (``residual_first``: act(conv2d(x, w) + bias + residual), a ResNet block's
    tail).  ``w2``: the weight as a [OC, Kp] fp32 matrix (K = C/groups*KH*KW
    zero-padded to 32), which the compiler keeps as a constant so its split
    planes are cached.  ``groups``: the image seen as N*groups images of
    C/groups channels (each group's channels are contiguous in NCHW), one
    batched GEMM per image over the groups (depthwise: groups = C)."""
    if not x.is_cuda:
        return conv2d_ref(x, w, bias, stride, padding, dilation, act, residual, residual_first, groups)
    dt = x.dtype
    xf = _f32(x).contiguous()
    N, C, H, W = xf.shape
    OC, Cg, KH, KW = w.shape
    G = groups
    if C != Cg * G or OC % G:
        raise ValueError(f"conv2d groups={G}: input channels {C} / weight {tuple(w.shape)} do not match")
    OCg = OC // G
    sh, sw = stride
    ph, pw = padding
    dh, dw = dilation
    OH = (H + 2 * ph - dh * (KH - 1) - 1) // sh + 1
    OW = (W + 2 * pw - dw * (KW - 1) - 1) // sw + 1
    K = Cg * KH * KW
    Kp = -(-K // 32) * 32
    if w2 is None:
        w2 = _pad_k(_f32(w).reshape(OC, K)).contiguous()
    if w2.shape != (OC, Kp) or w2.dtype != torch.float32:
        raise ValueError(f"conv weight matrix must be fp32 [{OC}, {Kp}]")
    P = OH * OW
    NG = N * G
    planes = torch.empty((2, NG * P, Kp), dtype=torch.float16, device=x.device)
    prinv = torch.empty((NG * P,), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    _lib.check(L.nos_im2col_h3(xf.data_ptr(), planes.data_ptr(), NG * P * Kp, prinv.data_ptr(), NG, Cg, H, W, KH, KW,
                               sh, sw, ph, pw, dh, dw, Kp, _stream()), "nos_im2col_h3")
    wp, wsc = split_f32_weight_h3(w2)
    out = torch.empty((N, OC, OH, OW), dtype=torch.float32, device=x.device)
    epi = _act_epi(act) | (EPI_BIAS_ROW if bias is not None else 0)
    if residual is not None:
        epi |= EPI_RESID_PRE if residual_first else EPI_RESID
    b = _f32(bias).contiguous() if bias is not None else None
    r = _f32(residual).contiguous() if residual is not None else None
    if r is not None and r.shape != out.shape:
        raise ValueError(f"residual must be {tuple(out.shape)}")
    if G == 1:
        # out[n] = W [OC, Kp] . patches[n]^T: A = the weight (shared, stride 0), W-operand = image n's patches
        _gemm_batched(wp, wsc, 0, 0, planes, prinv, P * Kp, P, out, OC, P, Kp, N, epi, bias=b, residual=r,
                      ldc=P, sc=OC * P, ldr=P, sr=OC * P)
    else:
        # per image: batch = the groups -- A = group g's weight rows, W-operand
        # = group g's patches (image n*G + g of the im2col), C = its OCg channels
        for n in range(N):
            _gemm_batched(wp, wsc, OCg * Kp, OCg, planes, prinv, P * Kp, P, out, OCg, P, Kp, G, epi,
                          bias=b, residual=r[n:] if r is not None else None, ldc=P, sc=OCg * P, ldr=P,
                          sr=OCg * P, sbias=OCg, c_off=n * OC * P, w_off=n * G * P * Kp, wr_off=n * G * P)
    return out if dt == torch.float32 else out.to(dt)


def patches(x: torch.Tensor, ph: int, pw: int, dtype: torch.dtype = torch.float32, hp: int | None = None,
            wp: int | None = None):
    """A ViT's patch rows of an fp32 NCHW image: [N, (H/ph)(W/pw), C ph pw]
    with columns (c, dy, dx), in ``dtype``.  On the GPU one im2col pass over
    the image (stride = kernel, no padding; a cropped view is read through
    its strides, no contiguous copy): fp32 under h3 math as the GEMM's A
    planes (:class:`ops.H3Planes`), bf16 as the GEMM's bf16 operand (the cast
    folded in); otherwise the PyTorch views + copy.  ``hp`` x ``wp`` patches
    from the image's top-left corner (default: as many as fit)."""
    from .. import ops

    N, C, H, W = x.shape
    hp = H // ph if hp is None else hp
    wp = W // pw if wp is None else wp
    if not (0 < hp * ph <= H and 0 < wp * pw <= W):
        raise ValueError(f"patches: {hp}x{wp} patches of {ph}x{pw} exceed the {H}x{W} image")
    K = C * ph * pw
    P = hp * wp
    bf = dtype == torch.bfloat16
    gpu = x.is_cuda and x.dtype == torch.float32 and (bf or (dtype == torch.float32 and ops.h3_planes_active()
                                                                and K % 32 == 0))
    if not gpu:
        x = x[:, :, :hp * ph, :wp * pw]
        y = x.reshape(N, C, hp, ph, wp, pw).permute(0, 2, 4, 1, 3, 5).reshape(N, P, K)
        return y.to(dtype)
    if x.stride(3) != 1:
        x = x.contiguous()
    sN, sC, sH = x.stride(0), x.stride(1), x.stride(2)
    if bf:
        out = torch.empty((N, P, K), dtype=torch.bfloat16, device=x.device)
        _lib.check(_lib.lib().nos_im2col(x.data_ptr(), sN, sC, sH, out.data_ptr(), 0, None, N, C, hp * ph, wp * pw, ph,
                                         pw, ph, pw, 0, 0, 1, 1, K, 1, _stream()), "nos_im2col")
        return out
    planes = torch.empty((2, N * P, K), dtype=torch.float16, device=x.device)
    prinv = torch.empty((N * P,), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().nos_im2col(x.data_ptr(), sN, sC, sH, planes.data_ptr(), N * P * K, prinv.data_ptr(), N, C,
                                     hp * ph, wp * pw, ph, pw, ph, pw, 0, 0, 1, 1, K, 0, _stream()), "nos_im2col")
    return ops.H3Planes(planes, prinv, 0.0, (N, P, K))


COLS_NCH = 32   # gemm_f32h.hip: row chunks of the column maxima (nos_split_cols_h3's work buffer)


def _split_cols_h3(x3: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The columns of fp32 x3 [nb, R, C] as h3 plane rows (``nos_split_cols_h3``):
    planes [2, nb * C, ceil32(R)] (zero-padded), 1 / row scale [nb * C] -- the
    split of x3's transpose without a transposed copy."""
    nb, R, C = x3.shape
    if x3.stride(-1) != 1 or (nb > 1 and x3.stride(0) < (R - 1) * x3.stride(1) + C):
        x3 = x3.contiguous()
    Rp = _pad_k_len(R)
    planes = torch.empty((2, nb * C, Rp), dtype=torch.float16, device=x3.device)
    rinv = torch.empty((nb * C,), dtype=torch.float32, device=x3.device)
    work = torch.empty((COLS_NCH * nb * C,), dtype=torch.float32, device=x3.device)
    _lib.check(_lib.lib().nos_split_cols_h3(x3.data_ptr(), x3.stride(1), x3.stride(0) if nb > 1 else 0, R, C, nb,
                                            planes.data_ptr(), Rp, planes[0].numel(), rinv.data_ptr(),
                                            work.data_ptr(), _stream()), "nos_split_cols_h3")
    return planes, rinv


def _rows_h3(x3: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The rows of fp32 x3 [nb, R, C] as h3 plane rows [2, nb * R, ceil32(C)]."""
    R, C = x3.shape[1:]
    x2 = _pad_k(x3).reshape(-1, _pad_k_len(C))
    return _split_rows_h3(x2 if x2.stride(-1) == 1 and x2.is_contiguous() else x2.contiguous(), ln=False)


def mm(a: torch.Tensor, b: torch.Tensor, a_t: bool = False, b_t: bool = False, bias: torch.Tensor | None = None,
       act: str | None = None, residual: torch.Tensor | None = None) -> torch.Tensor:
    """op(a) @ op(b) on the h3 batched GEMM, op(x) = x^T (last two dims) when
    the flag is set; batch dims equal, or one side 2-D.  A transposed A or a
    plain B operand is split by columns (``nos_split_cols_h3``), so no
    operand is ever copied into its transpose (training's dX = dY W and
    dW = dY^T X, attention's P V and P^T dO).  An unbatched product takes the
    GEMM's epilogue: ``bias`` [N], ``act`` (gelu / relu), then ``residual``
    [M, N] (contiguous fp32)."""
    if not a.is_cuda:
        A = a.transpose(-1, -2) if a_t else a
        B = b.transpose(-1, -2) if b_t else b
        y = A.float() @ B.float()
        if bias is not None:
            y = y + bias.float()
        y = _act(y, act)
        return (y if residual is None else y + residual.float()).to(a.dtype)
    dt = a.dtype
    M, K = (a.shape[-1], a.shape[-2]) if a_t else (a.shape[-2], a.shape[-1])
    N, Kb = (b.shape[-2], b.shape[-1]) if b_t else (b.shape[-1], b.shape[-2])
    ba, bb = a.shape[:-2], b.shape[:-2]
    if Kb != K or (ba and bb and ba != bb):
        raise ValueError(f"mm shapes: {tuple(a.shape)}{'^T' if a_t else ''} @ {tuple(b.shape)}{'^T' if b_t else ''}")
    bshape = ba or bb
    nb = math.prod(bshape) if bshape else 1
    a3, b3 = _f32(a).reshape(-1, *a.shape[-2:]), _f32(b).reshape(-1, *b.shape[-2:])
    ap, arinv = _split_cols_h3(a3) if a_t else _rows_h3(a3)      # A rows: op(a)'s M rows of K
    bp, brinv = _rows_h3(b3) if b_t else _split_cols_h3(b3)      # W rows: op(b)'s N columns of K
    Kp = ap.shape[2]
    out = torch.empty((nb, M, N), dtype=torch.float32, device=a.device)
    epi = _act_epi(act) | (EPI_BIAS if bias is not None else 0) | (EPI_RESID if residual is not None else 0)
    if epi and (nb != 1 or (residual is not None and (residual.shape != (M, N) or not residual.is_contiguous()
                                                        or residual.dtype != torch.float32))):
        raise ValueError("mm: the epilogue takes an unbatched product and a contiguous fp32 [M, N] residual")
    _gemm_batched(ap, arinv, M * Kp if ba else 0, M if ba else 0, bp, brinv, N * Kp if bb else 0, N if bb else 0,
                  out, M, N, Kp, nb, epi, bias=None if bias is None else bias.float().contiguous(), residual=residual)
    out = out.view(*bshape, M, N)
    return out if dt == torch.float32 else out.to(dt)


def matmul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [..., M, K] @ b [..., K, N]; batch dims equal, or one side 2-D."""
    return mm(a, b)


def _pad_k_len(k: int) -> int:
    return -(-k // 32) * 32


def linear_rms(x: torch.Tensor, wg: torch.Tensor, bias: torch.Tensor | None = None, act: str | None = None,
               eps: float = 1e-6, glu: bool = False, lora: tuple | None = None) -> torch.Tensor:
    """act(RMSNorm(x) @ (W * gamma)^T + b): the row statistics in the h3 split
    pre-pass (``nos_split_rows_h3`` mode 2), gamma folded into ``wg``.
    ``glu``: ``wg`` is a merged [gate; up] weight and the result is
    silu(gate) * up (the GEMV's epilogue for decode rows).  ``lora``: the
    adapter operand of :func:`gemv` -- decode rows on the GEMV only (an error otherwise)."""
    if lora is not None:
        x2l = x.reshape(-1, x.shape[-1])
        if x2l.stride(-1) != 1 or x2l.stride(0) % 4 or x2l.data_ptr() % 16:
            x2l = x2l.contiguous()
        if not gemv_ok(x2l, wg) or x2l.dtype != torch.float32:
            raise ValueError(f"linear_rms: the adapter epilogue exists on the GEMV only; x {tuple(x.shape)} {x.dtype} and "
                             f"W {tuple(wg.shape)} are not a product it takes (gemv_ok)")
        out = gemv(x2l, wg, bias, act, rms_eps=float(eps) or 1e-30, glu=glu, lora=lora)
        return out.view(*x.shape[:-1], wg.shape[0] // 2 if glu else wg.shape[0])
    if glu:
        x2g = _f32(x).reshape(-1, x.shape[-1])
        if not (x.is_cuda and x2g.shape[0] <= GEMV_MAX_ROWS and gemv_ok(x2g.contiguous(), wg)):
            y = linear_rms(x, wg, bias, act, eps)
            h = y.shape[-1] // 2
            return (F.silu(y[..., :h].float()) * y[..., h:].float()).to(y.dtype)
    if not x.is_cuda:
        return linear_rms_ref(x, wg, bias, act, eps)
    dt = x.dtype
    K = x.shape[-1]
    N = wg.shape[0]
    if K % 32:
        raise ValueError("native linear_rms needs K % 32 == 0")
    x2 = _f32(x).reshape(-1, K)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    M = x2.shape[0]
    if glu and not gemv_ok(x2, wg):
        x2 = x2.clone()   # an aligned copy: the GLU form exists only on the GEMV
    if M <= GEMV_MAX_ROWS and gemv_ok(x2, wg):   # a decode step: the RMS statistics in the GEMV's prologue
        out = gemv(x2, wg, bias, act, rms_eps=float(eps) or 1e-30, glu=glu)
        out = out.view(*x.shape[:-1], N // 2 if glu else N)
        return out if dt == torch.float32 else out.to(dt)
    planes = torch.empty((2, M, K), dtype=torch.float16, device=x.device)
    rinv = torch.empty((M,), dtype=torch.float32, device=x.device)
    eln = 14 - math.frexp(math.sqrt(K))[1]
    _lib.check(_lib.lib().nos_split_rows_h3(x2.data_ptr(), x2.stride(0), planes.data_ptr(), K, M * K, rinv.data_ptr(),
                                            M, K, 2, float(eps), eln, _stream()), "nos_split_rows_h3")
    wp, csc = split_f32_weight_h3(wg)
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    b = _f32(bias).contiguous() if bias is not None else None
    epi = _act_epi(act) | (EPI_BIAS if b is not None else 0)
    _gemm_batched(planes, rinv, 0, 0, wp, csc, 0, 0, out, M, N, K, 1, epi, bias=b)
    out = out.view(*x.shape[:-1], N)
    return out if dt == torch.float32 else out.to(dt)


_ROPE_BOUND: dict[int, tuple] = {}


def _rope_bound(cos: torch.Tensor, sin: torch.Tensor) -> float:
    key = id(cos)
    hit = _ROPE_BOUND.get(key)
    if hit is not None and hit[0] is sin and hit[1] == cos._version:
        return hit[2]
    b = float(cos.abs().max() + sin.abs().max())
    _ROPE_BOUND[key] = (sin, cos._version, b)
    return b


def _check_attn_shapes(what: str, q, k, v) -> None:
    B, Sq, H, D = q.shape
    Hkv = k.shape[2]
    if D not in (64, 128) or H % Hkv or v.shape != k.shape or k.shape[0] != B or k.shape[3] != D:
        raise ValueError(f"native {what}: head_dim 64/128, H % Hkv == 0; got q {tuple(q.shape)}, k {tuple(k.shape)}")


def _sdpa_fwd(what: str, q, k, v, causal, scale, rope=None, out=None, lse: bool = False):
    """The forward of :func:`sdpa` and :func:`sdpa_lse` on CUDA tensors:
    (o, the rows' log-sum-exp or None)."""
    _check_attn_shapes(what, q, k, v)
    B, Sq, H, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    if rope is not None and Sq > Skv:   # query i is rotated at position i + Skv - Sq: negative for the first rows
        raise ValueError(f"native {what}: rope needs Sq <= Skv, got Sq {Sq}, Skv {Skv}")
    (qf, ldq, bsq), (kf, ldk, bsk), (vf, ldv, bsv) = (_rows(t, aligned=True) for t in (q, k, v))
    if out is None or out.dtype != torch.float32:
        o = torch.empty((B, Sq, H, D), dtype=torch.float32, device=q.device)
    else:
        o = out
    L = _lib.lib()
    nbytes = int(L.nos_attn_h3g_workspace(B, H, Hkv, Sq, Skv, D))
    ws, wptr = _workspace(nbytes, q.device)
    rc_, rs_, rb = None, None, 0.0
    if rope is not None:
        rc_, rs_ = rope[0], rope[1]
        if rc_.dtype != torch.float32 or not rc_.is_contiguous() or rc_.shape != (Skv, D) or rs_.shape != (Skv, D):
            raise ValueError(f"rope tables must be contiguous fp32 [{Skv}, {D}]")
        rb = _rope_bound(rc_, rs_)
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    args = (qf.data_ptr(), ldq, bsq, kf.data_ptr(), ldk, bsk, vf.data_ptr(), ldv, bsv, o.data_ptr(), o.stride(1),
            o.stride(0), B, H, Hkv, Sq, Skv, D, int(bool(causal)), float(sc), _ptr(rc_), _ptr(rs_), float(rb), wptr,
            nbytes)
    ls = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device) if lse else None
    if lse:
        _lib.check(L.nos_attn_h3g_lse(*args, ls.data_ptr(), _stream()), "nos_attn_h3g_lse")
    else:
        _lib.check(L.nos_attn_h3g(*args, _stream()), "nos_attn_h3g")
    if out is not None and out is not o:
        out.copy_(o)
        return out, ls
    return (o if q.dtype == torch.float32 else o.to(q.dtype)), ls


def sdpa(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False, scale: float | None = None,
         rope: tuple | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """softmax(scale q k^T [causal]) v: q [B, Sq, H, D], k / v [B, Skv, Hkv, D]
    (heads contiguous per token; any token / batch strides, e.g. slices of a
    fused QKV projection), D = 64 or 128, H % Hkv == 0.  ``rope`` = (cos, sin)
    fp32 tables [Skv, D]: q (row i at position i + Skv - Sq, so Sq <= Skv) and
    k are rotated first (inside the kernels).
    ``out``: the tensor to fill (a non-fp32 one by copy)."""
    if not q.is_cuda:
        return sdpa_ref(q, k, v, causal, scale, rope)
    return _sdpa_fwd("sdpa", q, k, v, causal, scale, rope, out)[0]


# ------------------------------------------------------------------ training attention (attention_h3g_bwd.hip)
BWD_MAX_QSPLIT = 8   # attention_h3g_bwd.hip MAX_QSPLIT: ranges of the dK / dV sweep
BWD_ABS_ROWS = 256   # attn_kv_planes.h ABS_ROWS: rows per absmax chunk


def sdpa_bwd_workspace_bytes(B: int, H: int, Hkv: int, Sq: int, Skv: int, D: int) -> int:
    """Workspace bytes of :func:`sdpa_bwd` from the shapes alone (the memory
    estimate of a training tenant needs no library): equals
    ``nos_attn_h3g_bwd_workspace`` (attention_h3g_bwd.hip ``layout``)."""
    def al(x: int) -> int:
        return -(-x // 256) * 256

    skvp, sqp = -(-Skv // 32) * 32, -(-Sq // 32) * 32
    nck, ncq = -(-Skv // BWD_ABS_ROWS), -(-Sq // BWD_ABS_ROWS)
    return (al(B * Hkv * skvp * 4 * D * 2)          # K / V row planes
            + al(B * Hkv * skvp * 2 * D * 2)        # K transposed planes
            + 2 * al(B * H * sqp * 4 * D * 2)       # Q / dO row planes, transposed planes
            + al(B * H * sqp * 16)                  # per-row constants (delta, log-sum-exp, Q scale)
            + al(B * Hkv * nck * 2 * 4) + al(B * H * ncq * 2 * 4)   # absmax partials
            + al(B * Hkv * 2 * 4) + al(B * Hkv * 8 * 4)             # scales, per-group constants
            + BWD_MAX_QSPLIT * B * Skv * Hkv * 2 * D * 4)           # partial dK / dV of a split sweep


def sdpa_lse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False, scale: float | None = None):
    """:func:`sdpa` (no rotary) that also returns the rows' log-sum-exp for
    :func:`sdpa_bwd`: (o [B, Sq, H, D], lse fp32 [B, H, Sq]); the same O bits
    as :func:`sdpa` (``nos_attn_h3g_lse``)."""
    if not q.is_cuda:
        return sdpa_lse_ref(q, k, v, causal, scale)
    return _sdpa_fwd("sdpa_lse", q, k, v, causal, scale, lse=True)


def sdpa_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, o: torch.Tensor, lse: torch.Tensor, do: torch.Tensor,
             causal: bool = False, scale: float | None = None, out: tuple | None = None):
    """(dq, dk, dv) of :func:`sdpa_lse`'s o for the upstream gradient ``do``
    (``nos_attn_h3g_bwd``: two kernels that recompute P from ``lse``, no
    atomics -- the same bits on every call).  Tensors as in :func:`sdpa`,
    any token / batch strides; gradients contiguous, in the inputs' dtypes.
    ``out`` = (dq, dk, dv): fp32 CUDA tensors to write instead (heads
    contiguous per token; every element is overwritten, none is read)."""
    if not q.is_cuda:
        return sdpa_bwd_ref(q, k, v, o, lse, do, causal, scale)
    _check_attn_shapes("sdpa_bwd", q, k, v)
    B, Sq, H, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    if o.shape != q.shape or do.shape != q.shape or lse.shape != (B, H, Sq):
        raise ValueError(f"sdpa_bwd: o / do must be {tuple(q.shape)} and lse {(B, H, Sq)}")
    (qf, ldq, bsq), (kf, ldk, bsk), (vf, ldv, bsv), (of, ldo, bso), (dof, lddo, bsdo) = (
        _rows(t, aligned=True) for t in (q, k, v, o, do))
    lf = lse.float().contiguous()
    if out is not None:
        dq, dk, dv = out
        for t, ref in ((dq, q), (dk, k), (dv, k)):
            if t.shape != ref.shape or t.dtype != torch.float32 or not t.is_cuda or _rows(t, aligned=True)[0] is not t:
                raise ValueError("sdpa_bwd: out must be aligned fp32 CUDA tensors in the shapes of q, k, v")
    else:
        dq = torch.empty((B, Sq, H, D), dtype=torch.float32, device=q.device)
        dk = torch.empty((B, Skv, Hkv, D), dtype=torch.float32, device=q.device)
        dv = torch.empty((B, Skv, Hkv, D), dtype=torch.float32, device=q.device)
    nbytes = sdpa_bwd_workspace_bytes(B, H, Hkv, Sq, Skv, D)
    ws, wptr = _workspace(nbytes, q.device)
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    rc = _lib.lib().nos_attn_h3g_bwd(qf.data_ptr(), ldq, bsq, kf.data_ptr(), ldk, bsk, vf.data_ptr(), ldv, bsv,
                                     of.data_ptr(), ldo, bso, dof.data_ptr(), lddo, bsdo, lf.data_ptr(),
                                     dq.data_ptr(), dq.stride(1), dq.stride(0), dk.data_ptr(), dk.stride(1),
                                     dk.stride(0), dv.data_ptr(), dv.stride(1), dv.stride(0), B, H, Hkv, Sq, Skv, D,
                                     int(bool(causal)), float(sc), wptr, nbytes, _stream())
    _lib.check(rc, "nos_attn_h3g_bwd")
    if out is not None:
        return dq, dk, dv
    return tuple(t if x.dtype == torch.float32 else t.to(x.dtype) for t, x in ((dq, q), (dk, k), (dv, v)))


# ------------------------------------------------------------------ stateful decoding (decode.hip)
def _i32_pos(pos: torch.Tensor, B: int) -> torch.Tensor:
    if pos.dtype != torch.int32 or pos.shape != (B,) or not pos.is_contiguous():
        raise ValueError(f"positions must be a contiguous i32 [{B}] tensor, got {pos.dtype} {tuple(pos.shape)}")
    return pos


def _ring(what: str, window, limit, C: int, S: int, rope) -> bool:
    """``window`` / ``limit`` of a ring cache of C slots at a step of S rows: whether the cache is a ring."""
    from ..podserver.program.reference import _ring_args

    ring = _ring_args(what, window, limit, C, S)
    if ring and rope is not None and limit > rope[0].shape[0]:
        raise ValueError(f"{what}: limit {limit} exceeds the rotary tables' {rope[0].shape[0]} rows")
    return ring


def kv_write(cache: torch.Tensor, x: torch.Tensor, pos: torch.Tensor, rope: tuple | None = None,
             second: tuple | None = None, scales: torch.Tensor | None = None, deq: bool = False,
             window: int | None = None, limit: int | None = None):
    """cache[b, pos[b] + s] = x[b, s] in place (rows past the cache dropped);
    ``rope`` = (cos, sin) fp32 tables: x rotated at those positions first.
    ``second`` = (cache2, x2): a second, unrotated write of the same shape in
    the same launch (a layer's V beside its K).  Returns ``cache``.

    An int8 ``cache`` with its ``scales`` [B, L, H] (fp32; ``second`` then
    (cache2, x2, scales2)): the fp32 rows are quantized as they are written
    (after the rotation; ``quantize_rows_q8``'s rule per row).  ``deq``:
    also return the written rows as the cache now holds them, fp32
    [B, S, H, D] -- ``(cache, deq)``, with ``second`` ``(cache, deq, deq2)``.

    ``window`` and ``limit`` (together): the cache is a ring of C = L slots
    for a sliding window -- the row of position p goes to slot p % C, rows at
    p < 0 or p >= limit are dropped; min(limit, window + S - 1) <= C <= limit."""
    from ..podserver.program.reference import kv_write_ref, rotary_at_ref

    q8 = cache.dtype == torch.int8
    if q8 != (scales is not None) or (deq and not q8):
        raise ValueError("kv_write: an int8 cache, and only an int8 cache, takes scales (and gives deq)")
    ring = _ring("kv_write", window, limit, cache.shape[1], x.shape[1], rope)
    if q8:
        return _kv_write_q8(cache, x, pos, rope, second, scales, deq, window, limit)
    if not cache.is_cuda:
        if second is not None:
            kv_write_ref(second[0], second[1], pos, window=window, limit=limit)
        return kv_write_ref(cache, rotary_at_ref(x, rope[0], rope[1], pos) if rope else x, pos, window=window,
                            limit=limit)
    B, L, H, D = cache.shape
    S = x.shape[1]
    if x.shape[0] != B or x.shape[2:] != cache.shape[2:] or not cache.is_contiguous():
        raise ValueError(f"kv_write: x {tuple(x.shape)} does not fit the cache {tuple(cache.shape)}")
    x, ldx, bsx = _rows(x)
    c = s_ = None
    R = 0
    if rope is not None:
        c, s_ = rope[0].float().contiguous(), rope[1].float().contiguous()
        R = c.shape[0]
    x2p, ld2, bs2, c2p = None, 0, 0, None
    if second is not None:
        c2, x2 = second
        if c2.shape != cache.shape or c2.dtype != cache.dtype or x2.shape != x.shape or x2.dtype != x.dtype \
                or not c2.is_contiguous():
            raise ValueError("kv_write: the second write must match the first's shapes and dtypes")
        x2, ld2, bs2 = _rows(x2)
        x2p, c2p = x2.data_ptr(), c2.data_ptr()
    if ring:
        _lib.check(_lib.lib().nos_kv_write_ring(x.data_ptr(), _bf(x), ldx, bsx, cache.data_ptr(), _bf(cache),
                                                _i32_pos(pos, B).data_ptr(), _ptr(c), _ptr(s_), R, B, S, H, D, L, x2p,
                                                ld2, bs2, c2p, int(window), int(limit), _stream()),
                   "nos_kv_write_ring")
        return cache
    _lib.check(_lib.lib().nos_kv_write(x.data_ptr(), _bf(x), ldx, bsx, cache.data_ptr(), _bf(cache),
                                       _i32_pos(pos, B).data_ptr(), _ptr(c), _ptr(s_), R, B, S, H, D, L, x2p, ld2, bs2,
                                       c2p, _stream()), "nos_kv_write")
    return cache


def _q8_cache_ok(what: str, cache: torch.Tensor, scales: torch.Tensor) -> None:
    if (cache.dtype != torch.int8 or scales.dtype != torch.float32 or tuple(scales.shape) != tuple(cache.shape[:3])
            or not cache.is_contiguous() or not scales.is_contiguous() or scales.device != cache.device):
        raise ValueError(f"{what}: an int8 cache [B, L, H, D] with fp32 scales [B, L, H] (both contiguous) required, "
                         f"got {cache.dtype} {tuple(cache.shape)} and {scales.dtype} {tuple(scales.shape)}")


def _kv_write_q8(cache, x, pos, rope, second, scales, deq, window=None, limit=None):
    """:func:`kv_write` into int8 caches (decode.hip ``nos_kv_write_q8``; the eager reference on the CPU)."""
    from ..podserver.program.reference import dequantize_kv_rows, kv_write_ref, quantize_kv_rows, rotary_at_ref

    _q8_cache_ok("kv_write", cache, scales)
    if second is not None:
        if len(second) != 3:
            raise ValueError("kv_write: the second write into an int8 cache is (cache2, x2, scales2)")
        _q8_cache_ok("kv_write", second[0], second[2])
    if x.dtype != torch.float32 or (second is not None and second[1].dtype != torch.float32):
        raise ValueError("kv_write: int8 caches take fp32 rows")
    if not cache.is_cuda:
        xs = [rotary_at_ref(x, rope[0], rope[1], pos) if rope else x] + ([second[1]] if second is not None else [])
        kv_write_ref(cache, xs[0], pos, scales, window=window, limit=limit)
        if second is not None:
            kv_write_ref(second[0], xs[1], pos, second[2], window=window, limit=limit)
        return (cache, *(dequantize_kv_rows(*quantize_kv_rows(t)) for t in xs)) if deq else cache
    B, L, H, D = cache.shape
    S = x.shape[1]
    if x.shape[0] != B or x.shape[2:] != cache.shape[2:]:
        raise ValueError(f"kv_write: x {tuple(x.shape)} does not fit the cache {tuple(cache.shape)}")
    x, ldx, bsx = _rows(x)
    c = s_ = None
    R = 0
    if rope is not None:
        c, s_ = rope[0].float().contiguous(), rope[1].float().contiguous()
        R = c.shape[0]
    dq = torch.empty((B, S, H, D), dtype=torch.float32, device=x.device) if deq else None
    x2p, ld2, bs2, c2p, s2p, dq2 = None, 0, 0, None, None, None
    if second is not None:
        c2, x2, s2 = second
        if c2.shape != cache.shape or x2.shape != x.shape:
            raise ValueError("kv_write: the second write must match the first's shapes and dtypes")
        x2, ld2, bs2 = _rows(x2)
        x2p, c2p, s2p = x2.data_ptr(), c2.data_ptr(), s2.data_ptr()
        dq2 = torch.empty_like(dq) if deq else None
    if window is not None:
        _lib.check(_lib.lib().nos_kv_write_ring_q8(x.data_ptr(), ldx, bsx, cache.data_ptr(), scales.data_ptr(),
                                                   _ptr(dq), _i32_pos(pos, B).data_ptr(), _ptr(c), _ptr(s_), R, B, S,
                                                   H, D, L, x2p, ld2, bs2, c2p, s2p, _ptr(dq2), int(window),
                                                   int(limit), _stream()), "nos_kv_write_ring_q8")
    else:
        _lib.check(_lib.lib().nos_kv_write_q8(x.data_ptr(), ldx, bsx, cache.data_ptr(), scales.data_ptr(), _ptr(dq),
                                              _i32_pos(pos, B).data_ptr(), _ptr(c), _ptr(s_), R, B, S, H, D, L, x2p,
                                              ld2, bs2, c2p, s2p, _ptr(dq2), _stream()), "nos_kv_write_q8")
    if not deq:
        return cache
    return (cache, dq) if second is None else (cache, dq, dq2)


def rotary_at(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """rotate_half rotary of x [B, S, H, D] at positions pos[b] + s (table rows clamped)."""
    from ..podserver.program.reference import rotary_at_ref

    if not x.is_cuda:
        return rotary_at_ref(x, cos, sin, pos)
    B, S, H, D = x.shape
    x, ldx, bsx = _rows(x)
    c, s_ = cos.float().contiguous(), sin.float().contiguous()
    if c.shape[1] != D or s_.shape != c.shape:
        raise ValueError(f"rotary tables must be [positions, {D}]")
    out = torch.empty((B, S, H, D), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().nos_rotary_pos(x.data_ptr(), ldx, bsx, out.data_ptr(), _i32_pos(pos, B).data_ptr(),
                                         c.data_ptr(), s_.data_ptr(), c.shape[0], B, S, H, D, _bf(x), _stream()),
               "nos_rotary_pos")
    return out


class DecodePartials:
    """The decode attention's split partials (``sdpa_cache(partials=True)``):
    ws [B x Hkv, NS, G, D + 2] fp32 -- consumed by :func:`gemv_partials`,
    which combines them in its x staging (the combine launch folded into the
    O-projection).  ``shape``: the attention output's [B, 1, H, D]."""

    def __init__(self, ws, NS, G, Hkv, D, shape, dtype):
        self.ws, self.NS, self.G, self.Hkv, self.D, self.shape, self.dtype = ws, NS, G, Hkv, D, tuple(shape), dtype


DECODE_MAX_ROWS = 32   # decode.hip MAXR: the G x Sq rows one pass of the decode kernel holds


def cache_flash_rule(G: int, Sq: int, D: int, fp32: bool, env=None) -> bool:
    """Whether a ``sdpa_cache`` step of ``Sq`` tokens with ``G`` query heads per K / V head runs on the flash
    kernel over the caches: an fp32 tenant with fp32 caches (``fp32``), head_dim 64 or 128, and more rows than
    one pass of the decode kernel holds (``G x Sq > 32``).  ``NOS_AMD_CACHE_FLASH=0`` (``env``: the environment
    to read, ``os.environ`` by default) keeps the decode kernel everywhere."""
    import os

    if (os.environ if env is None else env).get("NOS_AMD_CACHE_FLASH", "1") == "0":
        return False
    return bool(fp32) and D in (64, 128) and G * Sq > DECODE_MAX_ROWS


def sdpa_cache_flash_workspace_bytes(B: int, H: int, Hkv: int, Sq: int, L: int, D: int) -> int:
    """Workspace bytes of ``sdpa_cache(flash=True)`` from the shapes alone (the memory estimate needs no
    library): equals ``nos_attn_h3g_cache_workspace`` (attention_h3g.hip ``layout``)."""
    def al(x: int) -> int:
        return -(-x // 256) * 256

    skvp = -(-L // 32) * 32
    return (al(B * Hkv * skvp * 4 * D * 2) + al(B * Hkv * -(-L // BWD_ABS_ROWS) * 2 * 4) + al(B * Hkv * 2 * 4)
            + 4 * B * Sq * H * (D + 2) * 4)     # planes, absmax partials, scales, MAX_SPLIT key-split partials


def _sdpa_cache_flash(q, kc, vc, pos, scale, rope, fresh, window, limit):
    """:func:`sdpa_cache` on the flash kernel over fp32 caches (``window`` None: plain caches)."""
    B, Sq, H, D = q.shape
    L, Hkv = kc.shape[1], kc.shape[2]
    if fresh is not None:   # the step's rows first, by kv_write's launch: the same bits in the caches
        kv_write(kc, fresh[0], pos, rope=rope, second=(vc, fresh[1]), window=window, limit=limit)
    q, ldq, bsq = _rows(q, aligned=True)
    c = s_ = None
    R = 0
    if rope is not None:
        c, s_ = rope[0].float().contiguous(), rope[1].float().contiguous()
        R = c.shape[0]
        if c.shape[1] != D or s_.shape != c.shape:
            raise ValueError(f"rotary tables must be [positions, {D}]")
    lib = _lib.lib()
    nbytes = int(lib.nos_attn_h3g_cache_workspace(B, H, Hkv, Sq, L, D))
    if nbytes < 0:
        raise ValueError(f"sdpa_cache: no flash kernel for q {tuple(q.shape)} over caches {tuple(kc.shape)}")
    ws, wptr = _workspace(nbytes, q.device)
    out = torch.empty((B, Sq, H, D), dtype=torch.float32, device=q.device)
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    args = (q.data_ptr(), ldq, bsq, kc.data_ptr(), vc.data_ptr(), _i32_pos(pos, B).data_ptr(), _ptr(c), _ptr(s_), R,
            out.data_ptr(), out.stride(1), out.stride(0), B, H, Hkv, Sq, L, D, float(sc), wptr, nbytes)
    if window is not None:
        _lib.check(lib.nos_attn_h3g_cache_ring(*args, int(window), int(limit), _stream()), "nos_attn_h3g_cache_ring")
    else:
        _lib.check(lib.nos_attn_h3g_cache(*args, _stream()), "nos_attn_h3g_cache")
    return out


def sdpa_cache(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, pos: torch.Tensor, scale: float | None = None,
               rope: tuple | None = None, fresh: tuple | None = None, sync: torch.Tensor | None = None,
               partials: bool = False, scales: tuple | None = None, window: int | None = None,
               limit: int | None = None, flash: bool | None = None):
    """Query i of sequence b, at position pos[b] + i, attends the cached keys
    0 .. pos[b] + i: q [B, Sq, H, D], caches [B, L, Hkv, D] (fp32 / bf16).
    ``rope`` = (cos, sin): q rotated at its positions inside the kernel.
    ``fresh`` = (k, v) [B, Sq, Hkv, D]: the step's own K / V rows, written
    into the caches at the positions (K rotated by ``rope``) by the same
    launch -- a ``kv_write`` pair folded in.  ``sync``: a zeroed int32
    device buffer of >= B x Hkv counters owned by the call site (the kernel
    leaves it zero): the split combine runs in the decode launch's last
    workgroup per K / V head instead of a launch of its own.  ``partials``
    (CUDA, fp32 q, one query token): no combine -- returns the splits'
    :class:`DecodePartials` for :func:`gemv_partials`.  The
    flash-decoding kernel (decode.hip) for CUDA tensors, fp32 math.

    int8 caches with ``scales`` = (kscales, vscales) [B, L, Hkv] fp32 (q and
    ``fresh`` fp32): the attention of the values ``float(q) * scale`` the
    caches hold; fresh rows are quantized into the caches and the scales (as
    :func:`kv_write` does) and attended as stored.

    ``window`` and ``limit`` (together): sliding-window attention over ring
    caches of C = L slots -- the query at position p attends the positions
    max(0, p - window + 1) .. p, position j living in slot j % C (written
    there by :func:`kv_write` with the same pair, or as ``fresh`` rows; rows
    at positions >= limit dropped).  min(limit, window + Sq - 1) <= C <=
    limit; a counter outside [0, limit) gives zero rows.  The partials carry
    the ring's split count.

    ``flash``: the h3 flash kernel over the caches (attention_h3g.hip
    ``nos_attn_h3g_cache`` / ``nos_attn_h3g_cache_ring``: the matrix pipes,
    work bounded by the counters) instead of the one-token decode kernel --
    fp32 q and caches, no ``sync`` or ``partials`` (``ValueError``
    otherwise); ``fresh`` rows are written first by :func:`kv_write`'s
    launch (the same bits in the caches).  ``False``: the decode kernel.
    ``None``: the compiler's rule (:func:`cache_flash_rule`: ``G x Sq > 32``,
    where the decode kernel needs more than one pass), which the compiler
    applies to a program's steps and passes on as ``True`` / ``False``; a
    direct call has no step to mark and keeps the decode kernel, whose bits
    its callers compare across ``sync``, ``partials``, rings and dtypes.
    The CPU path is ``sdpa_cache_ref`` either way."""
    from ..podserver.program.reference import kv_write_ref, rotary_at_ref, sdpa_cache_ref

    q8 = kc.dtype == torch.int8
    if q8 != (scales is not None):
        raise ValueError("sdpa_cache: int8 caches, and only int8 caches, take scales")
    if q8:
        _q8_cache_ok("sdpa_cache", kc, scales[0])
        _q8_cache_ok("sdpa_cache", vc, scales[1])
        if q.dtype != torch.float32 or (fresh is not None and fresh[0].dtype != torch.float32):
            raise ValueError("sdpa_cache: int8 caches take an fp32 q and fp32 fresh rows")
    ks, vs = scales if q8 else (None, None)
    ring = _ring("sdpa_cache", window, limit, kc.shape[1], q.shape[1], rope)
    if not q.is_cuda:
        if fresh is not None:
            kv_write_ref(kc, rotary_at_ref(fresh[0], rope[0], rope[1], pos) if rope else fresh[0], pos, ks,
                         window=window, limit=limit)
            kv_write_ref(vc, fresh[1], pos, vs, window=window, limit=limit)
        return sdpa_cache_ref(rotary_at_ref(q, rope[0], rope[1], pos) if rope else q, kc, vc, pos, scale, ks, vs,
                              window=window, limit=limit)
    B, Sq, H, D = q.shape
    L, Hkv = kc.shape[1], kc.shape[2]
    if (kc.shape != vc.shape or kc.dtype != vc.dtype or kc.shape[0] != B or kc.shape[3] != D or H % Hkv
            or D not in (64, 128) or not kc.is_contiguous() or not vc.is_contiguous()):
        raise ValueError(f"sdpa_cache: q {tuple(q.shape)} vs caches {tuple(kc.shape)}")
    if flash:
        if q.dtype != torch.float32 or kc.dtype != torch.float32 or sync is not None or partials:
            raise ValueError("sdpa_cache: flash needs fp32 q and caches (no bf16 / int8) and takes no sync or partials")
        return _sdpa_cache_flash(q, kc, vc, pos, scale, rope, fresh, window if ring else None, limit)
    q, ldq, bsq = _rows(q)
    c = s_ = None
    R = 0
    if rope is not None:
        c, s_ = rope[0].float().contiguous(), rope[1].float().contiguous()
        R = c.shape[0]
    L_ = _lib.lib()
    nb = int(L_.nos_attn_decode_workspace(B, H, Hkv, Sq, L, D))
    ws = torch.empty((max(nb, 4) // 4,), dtype=torch.float32, device=q.device)
    out = torch.empty((B, Sq, H, D), dtype=q.dtype, device=q.device)
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    kn = vn = None
    ldk = ldv = bsk = bsv = nbf = 0
    if fresh is not None:
        kn, vn = fresh
        if kn.shape != (B, Sq, Hkv, D) or vn.shape != kn.shape or kn.dtype != vn.dtype:
            raise ValueError(f"sdpa_cache: fresh K / V {tuple(kn.shape)} for q {tuple(q.shape)}")
        (kn, ldk, bsk), (vn, ldv, bsv) = _rows(kn), _rows(vn)
        nbf = _bf(kn)
    if sync is not None and (not sync.is_cuda or sync.dtype != torch.int32 or not sync.is_contiguous()
                             or sync.numel() < B * Hkv):
        raise ValueError(f"sdpa_cache: sync needs >= {B * Hkv} contiguous int32 device counters")
    if partials and (Sq != 1 or sync is not None or q.dtype != torch.float32):
        raise ValueError("sdpa_cache: partials need one fp32 query token and no sync")
    if ring:   # the plain entry points' arguments (L the ring's slots), then the window and the limit
        tail = (_ptr(kn), _ptr(vn), *(() if q8 else (nbf,)), ldk, bsk, ldv, bsv, Sq if fresh is not None else 0,
                _ptr(sync), sync.numel() if sync is not None else 0, int(bool(partials)), int(window), int(limit),
                _stream())
        if q8:
            _lib.check(L_.nos_attn_decode_ring_q8(q.data_ptr(), ldq, bsq, kc.data_ptr(), vc.data_ptr(), ks.data_ptr(),
                                                  vs.data_ptr(), _i32_pos(pos, B).data_ptr(), _ptr(c), _ptr(s_), R,
                                                  out.data_ptr(), B, H, Hkv, Sq, L, D, float(sc), ws.data_ptr(),
                                                  ws.numel() * 4, *tail), "nos_attn_decode_ring_q8")
        else:
            _lib.check(L_.nos_attn_decode_ring(q.data_ptr(), _bf(q), ldq, bsq, kc.data_ptr(), vc.data_ptr(), _bf(kc),
                                               _i32_pos(pos, B).data_ptr(), _ptr(c), _ptr(s_), R, out.data_ptr(),
                                               _bf(out), B, H, Hkv, Sq, L, D, float(sc), ws.data_ptr(),
                                               ws.numel() * 4, *tail), "nos_attn_decode_ring")
    elif q8:
        _lib.check(L_.nos_attn_decode_q8(q.data_ptr(), ldq, bsq, kc.data_ptr(), vc.data_ptr(), ks.data_ptr(),
                                         vs.data_ptr(), _i32_pos(pos, B).data_ptr(), _ptr(c), _ptr(s_), R,
                                         out.data_ptr(), B, H, Hkv, Sq, L, D, float(sc), ws.data_ptr(), ws.numel() * 4,
                                         _ptr(kn), _ptr(vn), ldk, bsk, ldv, bsv, Sq if fresh is not None else 0,
                                         _ptr(sync), sync.numel() if sync is not None else 0, int(bool(partials)),
                                         _stream()), "nos_attn_decode_q8")
    else:
        _lib.check(L_.nos_attn_decode(q.data_ptr(), _bf(q), ldq, bsq, kc.data_ptr(), vc.data_ptr(), _bf(kc),
                                      _i32_pos(pos, B).data_ptr(), _ptr(c), _ptr(s_), R, out.data_ptr(), _bf(out), B, H,
                                      Hkv, Sq, L, D, float(sc), ws.data_ptr(), ws.numel() * 4, _ptr(kn), _ptr(vn), nbf,
                                      ldk, bsk, ldv, bsv, Sq if fresh is not None else 0, _ptr(sync),
                                      sync.numel() if sync is not None else 0, int(bool(partials)), _stream()),
                   "nos_attn_decode")
    if partials:
        return DecodePartials(ws, (L + 127) // 128, H // Hkv, Hkv, D, (B, Sq, H, D), q.dtype)
    return out


def pos_update(pos: torch.Tensor, add: bool, n: int) -> torch.Tensor:
    """pos += n (``add``) or pos = n, in place; returns ``pos``."""
    if not pos.is_cuda:
        return pos.add_(n) if add else pos.fill_(n)
    _lib.check(_lib.lib().nos_pos_update(_i32_pos(pos, pos.shape[0]).data_ptr(), pos.shape[0], int(bool(add)), int(n),
                                         _stream()), "nos_pos_update")
    return pos


def argmax(x: torch.Tensor, pos: torch.Tensor | None = None, pos_n: int = 0) -> torch.Tensor:
    """Index of the maximum over the last dim (first on ties), i32.
    ``pos`` (i32, one counter per row of x): advanced by ``pos_n`` in the same
    launch (a decode step's closing ``pos_add`` folded in)."""
    if not x.is_cuda:
        if pos is not None:
            pos.add_(pos_n)
        return x.float().argmax(dim=-1).to(torch.int32)
    L = x.shape[-1]
    x2 = x.reshape(-1, L)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    if pos is not None and (pos.numel() != x2.shape[0] or pos.dtype != torch.int32 or not pos.is_contiguous()):
        raise ValueError(f"argmax: pos needs one i32 counter per row ({x2.shape[0]})")
    out = torch.empty(x.shape[:-1], dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().nos_argmax(x2.data_ptr(), _bf(x2), x2.shape[0], L, x2.stride(0), out.data_ptr(), _ptr(pos),
                                     int(pos_n), _stream()), "nos_argmax")
    return out


# ------------------------------------------------------------------ sampling
def philox4x32(counter, key) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., Random123): ``counter`` [..., 4] and
    ``key`` [..., 2] as uint32 (broadcast against each other) -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def sampling_ctl(temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0) -> np.ndarray:
    """The four i32 control words :func:`sample` reads from device memory:
    ``[temperature as fp32 bits, top_k, top_p as fp32 bits, seed]``.
    Temperature 0 is greedy whatever the rest (the defaults pack to four
    zeros but for top_p's 1.0); top_k 0 and top_p 1 switch those filters off."""
    def number(v, what, integer=False):
        ok = isinstance(v, int) if integer else isinstance(v, (int, float))
        if not ok or isinstance(v, bool):
            raise ValueError(f"sampling: {what} must be {'an int' if integer else 'a number'}, got {v!r}")
        return v

    t, p = float(number(temperature, "temperature")), float(number(top_p, "top_p"))
    k, s = number(top_k, "top_k", True), number(seed, "seed", True)
    if not math.isfinite(t) or t < 0:
        raise ValueError(f"sampling: temperature must be finite and >= 0, got {temperature!r}")
    if k < 0 or k >= 1 << 31:
        raise ValueError(f"sampling: top_k must be in [0, 2^31), got {top_k!r}")
    if not 0 < p <= 1:
        raise ValueError(f"sampling: top_p must be in (0, 1], got {top_p!r}")
    if not 0 <= s < 1 << 31:
        raise ValueError(f"sampling: seed must be in [0, 2^31), got {seed!r}")
    words = np.array([t, p], dtype=np.float32).view(np.int32)
    return np.array([words[0], k, words[1], s], dtype=np.int32)


def sample_row_ref(x: np.ndarray, ctl, row: int = 0, pos: int = 0) -> dict:
    """One row of :func:`sample` on the host, scores and masses in fp64 --
    the reference the kernel is compared with, and its contract:

    * greedy (``token`` = the first index of the maximum, NaN winning, 0 for
      an all ``-inf`` row) when the temperature is <= 0 or the maximum ``m``
      is NaN or infinite;
    * else ``z = (x - m) / T``, ``w = exp(z)``; top-k (0 < k < L) keeps
      ``x >= `` the k-th largest logit, ties and all; top-p (0 < p < 1), after
      it, keeps token i iff the w-mass of kept tokens with a LARGER logit is
      ``< p Z`` (Z: the kept mass), so equal logits stay or go together;
    * the draw is Gumbel-max: ``u = ((word >> 9) + 0.5) 2^-23`` from word
      ``i & 3`` of Philox4x32-10 at key ``(seed, row)``, counter
      ``(i >> 2, pos, 0, 0)``; the largest ``z - log(-log(u))`` of the kept
      tokens wins, the lower index on a tie.

    Returns ``token`` and, for the tests' exclusion rules, ``keep`` (bool
    [L]), ``gap`` (best minus second-best score; inf when greedy) and
    ``p_margin`` (the least ``|mass above / Z - p|`` over the top-k set; inf
    without top-p)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    L = x.shape[0]
    c = np.asarray(ctl, dtype=np.int32).reshape(4)
    T, p = (float(v) for v in c[[0, 2]].view(np.float32))
    k, seed = int(c[1]), int(c[3])
    nan = np.isnan(x)
    idx = int(np.argmax(nan)) if nan.any() else int(np.argmax(x))
    m = x[idx]
    res = {"token": idx, "keep": None, "gap": math.inf, "p_margin": math.inf}
    if not T > 0 or not np.isfinite(m):
        return res
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        z = (x - m) / T
        w = np.exp(z)
        keep = np.ones(L, dtype=bool)
        if 0 < k < L:
            keep = x >= np.partition(x, L - k)[L - k]
        if 0 < p < 1:
            vals, inv = np.unique(x[keep], return_inverse=True)            # ascending
            mass = np.bincount(inv, weights=w[keep], minlength=len(vals))
            above = np.concatenate([np.cumsum(mass[::-1])[::-1][1:], [0.0]])   # mass of the larger logits
            Z = mass[::-1].sum()
            res["p_margin"] = float(np.abs(above / Z - p).min())
            kept = np.zeros(L, dtype=bool)
            kept[np.flatnonzero(keep)] = (above < p * Z)[inv]
            keep = kept
        i = np.arange(L, dtype=np.uint32)
        words = philox4x32(np.stack([i[::4] >> 2, np.full_like(i[::4], np.uint32(pos & 0xFFFFFFFF)),
                                     np.zeros_like(i[::4]), np.zeros_like(i[::4])], axis=-1),
                           np.array([seed & 0xFFFFFFFF, row & 0xFFFFFFFF], dtype=np.uint32)).reshape(-1)[:L]
        u = ((words >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        score = np.where(keep, z - np.log(-np.log(u)), -np.inf)
    tok = int(np.argmax(score))
    rest = np.delete(score, tok)
    res.update(token=tok, keep=keep, gap=float(score[tok] - rest.max()) if L > 1 else math.inf)
    return res


def sample(x: torch.Tensor, ctl: torch.Tensor, pos: torch.Tensor | None = None, pos_n: int = 0) -> torch.Tensor:
    """One token per row of logits (the last dim), i32: drawn from
    ``softmax(x / temperature)`` restricted by top-k, then top-p, as the
    control words ``ctl`` (:func:`sampling_ctl`: 4 i32 on x's device, read
    when the kernel runs) say; all zero: exactly :func:`argmax`.  The
    contract is :func:`sample_row_ref`'s, which CPU tensors run.  ``pos``
    (i32, one counter per row): its value before this call keys the draw
    (0 without it), and it is advanced by ``pos_n`` in the same launch."""
    L = x.shape[-1]
    x2 = x.reshape(-1, L)
    if (ctl.dtype != torch.int32 or ctl.numel() != 4 or not ctl.is_contiguous() or ctl.device != x.device):
        raise ValueError("sample: ctl must be 4 contiguous i32 control words on x's device")
    if pos is not None and (pos.numel() != x2.shape[0] or pos.dtype != torch.int32 or not pos.is_contiguous()):
        raise ValueError(f"sample: pos needs one i32 counter per row ({x2.shape[0]})")
    if not x.is_cuda:
        xs, c = x2.float().numpy(), ctl.numpy()
        ps = pos.reshape(-1).tolist() if pos is not None else [0] * x2.shape[0]
        out = torch.tensor([sample_row_ref(xs[r], c, r, ps[r])["token"] for r in range(x2.shape[0])],
                           dtype=torch.int32).reshape(x.shape[:-1])
        if pos is not None:
            pos.add_(pos_n)
        return out
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    out = torch.empty(x.shape[:-1], dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().nos_sample(x2.data_ptr(), _bf(x2), x2.shape[0], L, x2.stride(0), out.data_ptr(), _ptr(pos),
                                     int(pos_n), ctl.data_ptr(), _stream()), "nos_sample")
    return out


# ------------------------------------------------------------------ stop ids and repetition penalty
STOP_CTL_WORDS, MAX_STOP_IDS = 8, 4


def stopping_ctl(stop_ids=(), pad_id: int | None = None, repetition_penalty: float = 1.0,
                 id_bound: int | None = None) -> np.ndarray:
    """The eight i32 control words the stopping ops read from device memory:
    ``[penalty as fp32 bits, pad_id, n_stop, stop0, stop1, stop2, stop3, 0]``
    (unused stop slots 0).  ``stop_ids``: at most four token ids that end a
    row; ``pad_id``: what a finished row emits from then on (default: the
    first stop id, 0 without one); ``repetition_penalty``: finite and > 0,
    1 = off.  ``id_bound``: stop and pad ids must lie in [0, id_bound).  The
    defaults pack to all zeros but for the penalty's 1.0, which the kernels
    treat as zero bits: no stop ids, no penalty."""
    if isinstance(stop_ids, int) and not isinstance(stop_ids, bool):
        stop_ids = [stop_ids]
    if not isinstance(stop_ids, (list, tuple)) or len(stop_ids) > MAX_STOP_IDS:
        raise ValueError(f"stopping: stop_ids must be a list of at most {MAX_STOP_IDS} token ids, got {stop_ids!r}")

    def token(v, what):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
            raise ValueError(f"stopping: {what} must be an int token id, got {v!r}")
        hi = (1 << 31) if id_bound is None else int(id_bound)
        if not 0 <= v < hi:
            raise ValueError(f"stopping: {what} must lie in [0, {hi}), got {v!r}")
        return int(v)

    stops = [token(v, "stop_ids") for v in stop_ids]
    pad = token(pad_id, "pad_id") if pad_id is not None else (stops[0] if stops else 0)
    p = repetition_penalty
    if not isinstance(p, (int, float)) or isinstance(p, bool) or not math.isfinite(p) or not p > 0:
        raise ValueError(f"stopping: repetition_penalty must be finite and > 0, got {p!r}")
    if not math.isfinite(float(np.float32(p))) or not float(np.float32(p)) > 0:
        raise ValueError(f"stopping: repetition_penalty must be a positive finite fp32, got {p!r}")
    bits = int(np.array([p], dtype=np.float32).view(np.int32)[0])
    return np.array([bits, pad, len(stops), *stops, *([0] * (MAX_STOP_IDS - len(stops))), 0], dtype=np.int32)


def _stop_ctl(ctl: torch.Tensor, like: torch.Tensor, what: str) -> torch.Tensor:
    if ctl.dtype != torch.int32 or ctl.numel() != STOP_CTL_WORDS or not ctl.is_contiguous() or ctl.device != like.device:
        raise ValueError(f"{what}: ctl must be {STOP_CTL_WORDS} contiguous i32 control words on the operands' device")
    return ctl


def _i32_rows(t: torch.Tensor, n: int, what: str) -> torch.Tensor:
    if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous i32 tensor of {n} elements, got {t.dtype} {tuple(t.shape)}")
    return t


def seen_mark(seen: torch.Tensor, ids: torch.Tensor, reset: bool = False, vocab: int | None = None) -> torch.Tensor:
    """seen [B, W] (i32 bitmaps: bit ``id & 31`` of word ``id >> 5`` stands for
    token ``id``; token 31 is word 0's sign bit) |= the ids [B, S] (i32) of
    each row, in place; ``reset``: every row cleared first.  Ids outside
    [0, vocab) (default and at most 32 W) are ignored.  Returns ``seen``."""
    if seen.dtype != torch.int32 or seen.dim() != 2 or not seen.is_contiguous():
        raise ValueError(f"seen_mark: seen must be a contiguous i32 [B, W] bitmap, got {seen.dtype} {tuple(seen.shape)}")
    B, W = seen.shape
    if ids.dtype != torch.int32 or ids.dim() != 2 or ids.shape[0] != B or ids.device != seen.device:
        raise ValueError(f"seen_mark: ids must be i32 [{B}, S] on seen's device, got {ids.dtype} {tuple(ids.shape)}")
    vocab = 32 * W if vocab is None else int(vocab)
    if not 0 < vocab <= 32 * W:
        raise ValueError(f"seen_mark: vocab must lie in [1, {32 * W}], got {vocab}")
    if not seen.is_cuda:
        if reset:
            seen.zero_()
        idl = ids.to(torch.int64)
        bits = torch.zeros((B, 32 * W), dtype=torch.bool)
        ok = (idl >= 0) & (idl < vocab)
        rows = torch.arange(B).view(B, 1).expand_as(idl)
        bits[rows[ok], idl[ok]] = True
        words = (bits.view(B, W, 32).to(torch.int64) << torch.arange(32)).sum(-1)       # 0 .. 2^32 - 1
        seen |= torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)
        return seen
    if ids.stride(1) != 1:
        ids = ids.contiguous()
    _lib.check(_lib.lib().nos_seen_mark(seen.data_ptr(), B, W, ids.data_ptr(), ids.shape[1], ids.stride(0), vocab,
                                        int(bool(reset)), _stream()), "nos_seen_mark")
    return seen


def seen_bits(seen: torch.Tensor, vocab: int) -> torch.Tensor:
    """The bitmaps [B, W] as a bool mask [B, vocab]."""
    w = seen.to(torch.int64).cpu()
    return ((w[:, :, None] >> torch.arange(32)) & 1).bool().view(seen.shape[0], -1)[:, :vocab]


def penalize(x: torch.Tensor, seen: torch.Tensor, ctl: torch.Tensor) -> torch.Tensor:
    """The logits x [..., V] under the repetition penalty p of the control
    words ``ctl`` (:func:`stopping_ctl`; read on the device), a new tensor of
    x's shape and dtype: ``x`` where the row's bit in ``seen`` [rows, ceil(V /
    32)] is clear, else ``x * p`` for ``x < 0`` and ``x / p`` otherwise -- fp32
    math with a true division, bf16 logits rounded once; penalty bits 0 or
    p = 1: an exact copy.  x is only read, so a token seen twice is penalised
    once (transformers' gather / scatter)."""
    L = x.shape[-1]
    x2 = x.reshape(-1, L)
    rows, W = x2.shape[0], -(-L // 32)
    if seen.dtype != torch.int32 or tuple(seen.shape) != (rows, W) or not seen.is_contiguous() or seen.device != x.device:
        raise ValueError(f"penalize: seen must be a contiguous i32 [{rows}, {W}] bitmap on x's device, got "
                         f"{seen.dtype} {tuple(seen.shape)}")
    _stop_ctl(ctl, x, "penalize")
    if not x.is_cuda:
        _bf(x)
        p = ctl[:1].view(torch.float32) if int(ctl[0]) else torch.ones(1)
        xf = x2.float()
        hit = seen_bits(seen, L) & bool(p.item() != 1.0)
        return torch.where(hit, torch.where(xf < 0, xf * p, xf / p), xf).to(x.dtype).reshape(x.shape)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    out = torch.empty((rows, L), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().nos_penalize(x2.data_ptr(), _bf(x2), rows, L, x2.stride(0), out.data_ptr(), L,
                                       seen.data_ptr(), W, ctl.data_ptr(), _stream()), "nos_penalize")
    return out.reshape(x.shape)


def stop_step(next_ids: torch.Tensor | None, pos: torch.Tensor | None, done: torch.Tensor,
              ctl: torch.Tensor | None, n: int = 1, mode: int = 7) -> torch.Tensor | None:
    """The closing steps of a stopping program over B rows in one launch;
    each row's ``done`` flag is read first, then (``mode`` bits):

    * 1 -- ``stop_ids``: the returned ids (next_ids' shape) are ``pad_id``
      for a finished row, else ``next_ids``;
    * 2 -- ``pos_add(pos, done)``: ``pos += n`` for unfinished rows, in place;
    * 4 -- ``done_mark``: ``done |= id in the stop ids`` in place (id: what 1
      returned, or ``next_ids`` itself without 1).

    ``ctl``: :func:`stopping_ctl`'s words on the device.  Returns the ids
    (mode 1) or None."""
    B = done.numel()
    _i32_rows(done, B, "stop_step: done")
    if mode & 5:
        _i32_rows(next_ids, B, "stop_step: next ids")
        _stop_ctl(ctl, done, "stop_step")
    if mode & 2:
        _i32_rows(pos, B, "stop_step: pos")
    if not 0 < mode <= 7 or n < 0:
        raise ValueError(f"stop_step: mode {mode}, n {n}")
    if not done.is_cuda:
        d = done.reshape(-1) != 0
        ids = next_ids.reshape(-1).clone() if mode & 5 else None
        c = ctl.tolist() if mode & 5 else None
        if mode & 1:
            ids[d] = c[1]
        if mode & 2:
            pos += (~d).to(torch.int32).view(pos.shape) * int(n)
        if mode & 4:
            stops = torch.tensor(c[3:3 + min(max(c[2], 0), MAX_STOP_IDS)], dtype=torch.int32)
            done |= torch.isin(ids, stops).to(torch.int32).view(done.shape)
        return ids.view(next_ids.shape) if mode & 1 else None
    out = torch.empty_like(next_ids) if mode & 1 else None
    _lib.check(_lib.lib().nos_stop_step(_ptr(next_ids) if mode & 5 else None, _ptr(out),
                                        _ptr(pos) if mode & 2 else None, done.data_ptr(),
                                        _ptr(ctl) if mode & 5 else None, B, int(n), int(mode), _stream()),
               "nos_stop_step")
    return out


def stop_ids(next_ids: torch.Tensor, done: torch.Tensor, ctl: torch.Tensor) -> torch.Tensor:
    """``done[b] ? pad_id : next_ids[b]`` (:func:`stop_step`, mode 1)."""
    return stop_step(next_ids, None, done, ctl, mode=1)


def done_mark(done: torch.Tensor, ids: torch.Tensor, ctl: torch.Tensor) -> torch.Tensor:
    """``done[b] |= ids[b] is a stop id`` in place (:func:`stop_step`, mode 4); returns ``done``."""
    stop_step(ids, None, done, ctl, mode=4)
    return done


# ------------------------------------------------------------------ speculative decoding (n-gram drafts)
SPEC_CTL_WORDS, SPEC_MAX_K, SPEC_NGRAM = 4, 8, 3


def speculate_ctl(end: int = 0) -> np.ndarray:
    """The four i32 control words a speculating tenant's verify step reads from
    device memory: ``[end, 0, 0, 0]``.  ``end`` > 0: no step advances a row's
    counter past ``end``; 0: no bound but the cache."""
    if not isinstance(end, (int, np.integer)) or isinstance(end, bool) or not 0 <= end < 1 << 31:
        raise ValueError(f"speculate: end must be an int in [0, 2^31), got {end!r}")
    return np.array([int(end), 0, 0, 0], dtype=np.int32)


def _spec_hist(hist: torch.Tensor, what: str) -> torch.Tensor:
    if hist.dtype != torch.int32 or hist.dim() != 2 or not hist.is_contiguous() or hist.shape[1] > 1 << 28:
        raise ValueError(f"{what}: hist must be a contiguous i32 [B, L <= 2^28] tensor, got {hist.dtype} "
                         f"{tuple(hist.shape)}")
    return hist


def _spec_ids(t: torch.Tensor, B: int, like: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != B or t.device != like.device:
        raise ValueError(f"{what} must be i32 [{B}, n] on the operands' device, got {t.dtype} {tuple(t.shape)}")
    return t if t.stride(1) == 1 or t.shape[1] == 1 else t.contiguous()


def hist_write(hist: torch.Tensor, pos: torch.Tensor, ids: torch.Tensor, tail: torch.Tensor | None = None,
               n: torch.Tensor | None = None, back: int = 0, lead: int | None = None) -> torch.Tensor:
    """hist [B, L] (i32: the tokens of each row's sequence by position), in
    place: from ``base = pos[b] - back`` on, the first ``lead`` (default: all)
    columns of ``ids`` [B, S], then the columns of ``tail`` [B, T] -- with
    ``n`` [B] only its first ``n[b]``, and nothing at all for a row whose
    ``n[b]`` is 0.  Every index outside [0, L) is dropped.  Returns ``hist``."""
    _spec_hist(hist, "hist_write")
    B, L = hist.shape
    _i32_pos(pos, B)
    ids = _spec_ids(ids, B, hist, "hist_write: ids")
    lead = ids.shape[1] if lead is None else int(lead)
    if not 0 <= lead <= ids.shape[1] or back < 0:
        raise ValueError(f"hist_write: lead {lead} of {ids.shape[1]} columns, back {back}")
    T = 0
    if tail is not None:
        tail = _spec_ids(tail, B, hist, "hist_write: tail")
        T = tail.shape[1]
    if n is not None:
        _i32_pos(n, B)
    if not hist.is_cuda:
        for b in range(B):
            cnt = T
            if n is not None:
                if int(n[b]) <= 0:
                    continue
                cnt = min(int(n[b]), T)
            vals = ids[b, :lead].tolist() + (tail[b, :cnt].tolist() if cnt else [])
            base = int(pos[b]) - back
            for s, v in enumerate(vals):
                if 0 <= base + s < L:
                    hist[b, base + s] = v
        return hist
    _lib.check(_lib.lib().nos_hist_write(hist.data_ptr(), B, L, pos.data_ptr(), int(back), ids.data_ptr(), lead,
                                         ids.stride(0), _ptr(tail), T, tail.stride(0) if T else 0, _ptr(n),
                                         _stream()), "nos_hist_write")
    return hist


def _spec_launch(mode, hist, pos, ids, g, ctl, n_acc, out, B, L, K):
    _lib.check(_lib.lib().nos_spec_step(_ptr(hist), B, L, pos.data_ptr(), _ptr(ids), _ptr(g), _ptr(ctl), _ptr(n_acc),
                                        _ptr(out), K, mode, _stream()), "nos_spec_step")


def _spec_pair(ids: torch.Tensor, g: torch.Tensor, pos: torch.Tensor, ctl: torch.Tensor, what: str):
    B = pos.numel()
    _i32_pos(pos, B)
    if ids.dtype != torch.int32 or ids.dim() != 2 or ids.shape[0] != B or not 2 <= ids.shape[1] <= SPEC_MAX_K:
        raise ValueError(f"{what}: ids must be i32 [{B}, 2 <= K <= {SPEC_MAX_K}], got {ids.dtype} {tuple(ids.shape)}")
    if g.dtype != torch.int32 or g.shape != ids.shape:
        raise ValueError(f"{what}: the drawn ids must be i32 {tuple(ids.shape)}, got {g.dtype} {tuple(g.shape)}")
    if (ctl.dtype != torch.int32 or ctl.numel() != SPEC_CTL_WORDS or not ctl.is_contiguous()
            or not ctl.device == pos.device == ids.device == g.device):
        raise ValueError(f"{what}: ctl must be {SPEC_CTL_WORDS} contiguous i32 control words on the operands' device")
    return ids.contiguous(), g.contiguous()


def spec_accept(ids: torch.Tensor, g: torch.Tensor, pos: torch.Tensor, ctl: torch.Tensor, limit: int) -> torch.Tensor:
    """How far a verify step advances each row, ``m`` [B] (i32).  ``ids`` [B,
    K]: the pending token at position ``p = pos[b]`` and K - 1 drafts for p +
    1 ..; ``g`` [B, K]: the model's draw after each of them.  ``a`` = the
    leading j in 1 .. K - 1 with ``ids[b, j] == g[b, j - 1]`` (a match after
    a mismatch does not count); ``m = min(a + 1, limit - 1 - p, end - p if end
    > 0)`` floored at 0, ``end = ctl[0]``; a ``p`` outside [0, limit) gives 0."""
    ids, g = _spec_pair(ids, g, pos, ctl, "spec_accept")
    B, K = ids.shape
    if limit < 1:
        raise ValueError(f"spec_accept: limit {limit}")
    if not pos.is_cuda:
        end = int(ctl[0])
        out = torch.zeros(B, dtype=torch.int32)
        for b in range(B):
            p = int(pos[b])
            if not 0 <= p < limit:
                continue
            a = 0
            while a + 1 < K and int(ids[b, a + 1]) == int(g[b, a]):
                a += 1
            m = min(a + 1, limit - 1 - p)
            if end > 0:
                m = min(m, end - p)
            out[b] = max(m, 0)
        return out
    out = torch.empty(B, dtype=torch.int32, device=pos.device)
    _spec_launch(1, None, pos, ids, g, ctl, out, None, B, int(limit), K)
    return out


def pos_advance(pos: torch.Tensor, n: torch.Tensor) -> torch.Tensor:
    """``pos[b] += n[b]`` in place (a verify step's data-dependent advance); returns ``pos``."""
    B = pos.numel()
    _i32_pos(pos, B)
    _i32_pos(n, B)
    if not pos.is_cuda:
        return pos.add_(n)
    _spec_launch(4, None, pos, None, None, None, n, None, B, 1, 2)
    return pos


def spec_draft(hist: torch.Tensor, pos: torch.Tensor, k: int) -> torch.Tensor:
    """The next verify step's input [B, k] (i32) by n-gram lookup in the row's
    own history.  ``p = pos[b]``; column 0 is the pending token ``hist[b,
    p]``.  For n = 3, 2, 1 (each only if p >= n): the largest ``t < p`` with
    ``hist[t - n + 1 .. t] == hist[p - n + 1 .. p]``; the first n with a match
    wins and draft j (1 .. k - 1) is ``hist[t + j]`` if ``t + j <= p``, else
    the pending token.  No match: every draft is the pending token.  A ``p``
    outside [0, L): zeros."""
    _spec_hist(hist, "spec_draft")
    B, L = hist.shape
    _i32_pos(pos, B)
    if not 2 <= k <= SPEC_MAX_K or pos.device != hist.device:
        raise ValueError(f"spec_draft: k must be in [2, {SPEC_MAX_K}] (got {k}), pos on hist's device")
    if not hist.is_cuda:
        out = torch.zeros((B, k), dtype=torch.int32)
        for b in range(B):
            p = int(pos[b])
            if not 0 <= p < L:
                continue
            h = hist[b, :p + 1].tolist()
            out[b] = h[p]
            for n in range(min(SPEC_NGRAM, p), 0, -1):
                t = next((t for t in range(p - 1, n - 2, -1) if h[t - n + 1:t + 1] == h[p - n + 1:p + 1]), None)
                if t is not None:
                    for j in range(1, k):
                        if t + j <= p:
                            out[b, j] = h[t + j]
                    break
        return out
    out = torch.empty((B, k), dtype=torch.int32, device=hist.device)
    _spec_launch(8, hist, pos, None, None, None, None, out, B, L, k)
    return out


def spec_step(hist: torch.Tensor, pos: torch.Tensor, ids: torch.Tensor, g: torch.Tensor,
              ctl: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """A verify step's close in one launch, a workgroup per row:
    ``m = spec_accept(ids, g, pos, ctl, L)``; a row with m > 0 writes
    ``hist[b, p] = ids[b, 0]``, ``hist[b, p + 1 .. p + m] = g[b, 0 .. m - 1]``
    and ``pos[b] = p + m`` (both in place; m = 0 leaves the row alone); then
    ``spec_draft(hist, pos, K)``.  Returns (the next input [B, K], m [B])."""
    _spec_hist(hist, "spec_step")
    B, L = hist.shape
    ids, g = _spec_pair(ids, g, pos, ctl, "spec_step")
    if pos.numel() != B or hist.device != pos.device:
        raise ValueError(f"spec_step: hist {tuple(hist.shape)} and pos {tuple(pos.shape)} must share rows and device")
    K = ids.shape[1]
    if not hist.is_cuda:
        m = spec_accept(ids, g, pos, ctl, L)
        hist_write(hist, pos, ids, g, m, lead=1)
        pos_advance(pos, m)
        return spec_draft(hist, pos, K), m
    m = torch.empty(B, dtype=torch.int32, device=hist.device)
    out = torch.empty((B, K), dtype=torch.int32, device=hist.device)
    _spec_launch(15, hist, pos, ids, g, ctl, m, out, B, L, K)
    return out, m


GEMV_MAX_ROWS = 8
GEMV_X_BYTES = 65536   # the x rows the GEMV kernels stage in LDS: rows * K * 4 bytes at the most (gemv_ok, gemv_q8_ok)
EPI_SILU = 64 # csrc/hip/epilogue.h; decode.hip's GEMV: SiLU epilogue
EPI_GLU = 256  # decode.hip's GEMV: W = [gate; up], y = silu(gate) * up


# ------------------------------------------------------------------ multi-adapter LoRA
LORA_MAX_RANK = 64   # the stacked rank R of one adapted activation (decode.hip LORA_MAX_R)


def _lora_rows(sel: torch.Tensor, n: int, M: int, rps: int):
    """Per row m of M: (a valid adapter?, its index a - 1 clamped) for a = sel[m // rps]; no host read."""
    a = sel.to(torch.long).repeat_interleave(int(rps))[:M]
    return (a >= 1) & (a <= n), (a - 1).clamp(0, n - 1)


def lora_ref(x, A, B, sel, dtype: torch.dtype | None = None):
    """What ``lora(x, A, B, sel)`` means: for sequence b of x [batch, S, K] with a = ``sel[b]``,
    ``(x[b] @ A[a - 1].T) @ B[a - 1].T`` when a lies in [1, n] and zeros otherwise (0: the base
    model); A [n, R, K], B [n, N, R].  In ``dtype`` arithmetic (default: x's); the adapter is chosen
    by ``index_select`` on ``sel``, never read on the host."""
    dt = dtype or x.dtype
    n = A.shape[0]
    ok, idx = _lora_rows(sel, n, x.shape[0], 1)
    rows = []
    for b in range(x.shape[0]):
        Ab = A.index_select(0, idx[b:b + 1])[0].to(dt)
        Bb = B.index_select(0, idx[b:b + 1])[0].to(dt)
        rows.append((x[b].to(dt) @ Ab.T) @ Bb.T)
    y = torch.stack(rows)
    return torch.where(ok.view(-1, 1, 1), y, torch.zeros_like(y))


def lora_shrink_ref(x2, A, sel, rows_per_seq: int = 1, rms_eps: float = 0.0, gamma=None,
                    dtype: torch.dtype = torch.float32):
    """:func:`lora_shrink` in ``dtype`` arithmetic: t [M, R], row m = A[a_m - 1] @ x'[m] with
    ``a_m = sel[m // rows_per_seq]`` (zeros for an a_m outside [1, n]) and x' = x, RMS-normalised and
    times ``gamma`` when ``rms_eps`` > 0."""
    xf = x2.to(dtype)
    if rms_eps:
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + rms_eps)
        if gamma is not None:
            xf = xf * gamma.to(dtype)
    ok, idx = _lora_rows(sel, A.shape[0], xf.shape[0], rows_per_seq)
    t = torch.bmm(A.index_select(0, idx).to(dtype), xf.unsqueeze(-1)).squeeze(-1)
    return torch.where(ok.view(-1, 1), t, torch.zeros_like(t))


def lora_expand_ref(t, B, sel, rows_per_seq: int = 1, dtype: torch.dtype = torch.float32):
    """The adapter epilogue's delta [M, N]: row m = B[a_m - 1] @ t[m], zeros for a base row."""
    ok, idx = _lora_rows(sel, B.shape[0], t.shape[0], rows_per_seq)
    d = torch.bmm(B.index_select(0, idx).to(dtype), t.to(dtype).unsqueeze(-1)).squeeze(-1)
    return torch.where(ok.view(-1, 1), d, torch.zeros_like(d))


def _parts_args(p: "DecodePartials | None") -> tuple:
    return (None, 0, 0, 0, 0, 0) if p is None else (p.ws.data_ptr(), p.ws.numel(), p.NS, p.G, p.Hkv, p.D)


def lora_shrink(x, A: torch.Tensor, sel: torch.Tensor, rows_per_seq: int = 1, rms_eps: float = 0.0,
                gamma: torch.Tensor | None = None) -> torch.Tensor:
    """t [M, R] fp32 of the GEMV that follows: ``t[m] = A[sel[m // rows_per_seq] - 1] @ x'[m]`` for x [M, K]
    fp32 (M <= 8; a :class:`DecodePartials`: the decode attention's output, combined as that GEMV
    combines it) and A [n, R, K] fp32 -- one launch per adapted activation (decode.hip
    ``nos_lora_shrink``); x' is x under the GEMV's RMSNorm prologue (``rms_eps`` > 0, ``gamma``).
    Rows whose adapter is outside [1, n] are zeros.  CPU tensors: :func:`lora_shrink_ref`."""
    parts = x if isinstance(x, DecodePartials) else None
    n, R, K = A.shape
    if parts is None and not x.is_cuda:
        return lora_shrink_ref(x.reshape(-1, K), A, sel, rows_per_seq, rms_eps, gamma)
    if parts is not None:
        M = parts.shape[0]
        if parts.shape[2] * parts.shape[3] != K:
            raise ValueError(f"lora_shrink: A {tuple(A.shape)} for partials of {parts.shape}")
        x2 = None
    else:
        x2 = x.reshape(-1, K)
        if x2.stride(-1) != 1 or x2.stride(0) % 4 or x2.data_ptr() % 16:
            x2 = x2.contiguous()
        M = x2.shape[0]
        if x2.dtype != torch.float32:
            raise ValueError(f"lora_shrink takes an fp32 x, got {x2.dtype}")
    if (A.dtype != torch.float32 or A.stride(-1) != 1 or sel.dtype != torch.int32 or not sel.is_contiguous()
            or sel.numel() * int(rows_per_seq) < M or M > GEMV_MAX_ROWS or R % 4 or not 4 <= R <= LORA_MAX_RANK):
        raise ValueError(f"lora_shrink: A {tuple(A.shape)} {A.dtype} (fp32 [n, R <= {LORA_MAX_RANK}, K], R % 4 == 0), "
                         f"sel {tuple(sel.shape)} {sel.dtype} (i32, an id per {rows_per_seq} of the {M} <= "
                         f"{GEMV_MAX_ROWS} rows)")
    g = None if gamma is None else gamma.float().contiguous()
    t = torch.empty((M, R), dtype=torch.float32, device=A.device)
    _lib.check(_lib.lib().nos_lora_shrink(_ptr(x2), x2.stride(0) if x2 is not None else K, *_parts_args(parts),
                                          A.data_ptr(), A.stride(0), A.stride(1), sel.data_ptr(), n, int(rows_per_seq),
                                          _ptr(g), float(rms_eps), t.data_ptr(), M, R, K, _stream()), "nos_lora_shrink")
    return t


def _lora_args(lora: tuple, M: int, N: int) -> tuple:
    """The adapter operand ``(t [M, R], B [n, N, R], sel, rows_per_seq)`` of a GEMV as the entry points take it."""
    t, B, sel, rps = lora
    if (t.dtype != torch.float32 or B.dtype != torch.float32 or sel.dtype != torch.int32 or B.dim() != 3
            or B.shape[1] != N or tuple(t.shape) != (M, B.shape[2]) or not t.is_contiguous() or B.stride(-1) != 1
            or not sel.is_contiguous() or sel.numel() * int(rps) < M):
        raise ValueError(f"lora: t {tuple(t.shape)} {t.dtype}, B {tuple(B.shape)} {B.dtype} and sel {tuple(sel.shape)} "
                         f"{sel.dtype} are not the adapter operand of a [{M}, {N}] GEMV (t [M, R] and B [n, N, R] "
                         f"fp32, sel i32 with an id per {rps} rows)")
    return (t.data_ptr(), B.data_ptr(), B.stride(0), B.stride(1), sel.data_ptr(), B.shape[2], B.shape[0], int(rps))


def gemv_ok(x2: torch.Tensor, w: torch.Tensor) -> bool:
    """Whether the skinny-GEMM kernel takes this [M, K] x [N, K] product."""
    M, K = x2.shape
    return (x2.is_cuda and 0 < M <= GEMV_MAX_ROWS and K % 4 == 0 and M * K * 4 <= 65536 and x2.stride(-1) == 1
            and w.stride(-1) == 1 and x2.stride(0) % 4 == 0 and w.stride(0) % 4 == 0
            and x2.dtype in (torch.float32, torch.bfloat16) and w.dtype in (torch.float32, torch.bfloat16)
            and x2.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0)


def gemv(x2: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, act: str | None = None,
         residual: torch.Tensor | None = None, out: torch.Tensor | None = None, rms_eps: float = 0.0,
         glu: bool = False, lora: tuple | None = None) -> torch.Tensor:
    """y [M, N] = act(rms(x) [M, K] W^T + b) + R for M <= 8 (:func:`gemv_ok`):
    the weight-streaming kernel of a decode step, exact fp32 math; y, R in
    x's dtype, bias in W's.  ``rms_eps`` > 0: x rows RMS-normalised first
    (RMSNorm folded into the GEMM, gamma in W).  ``lora`` = (t, B, sel,
    rows_per_seq), fp32 x and W: the product gets ``+ B[sel[m // rows_per_seq]
    - 1] @ t[m]`` before anything else of the epilogue (t: :func:`lora_shrink`;
    a row whose adapter is 0 is the plain call's bit for bit)."""
    M, K = x2.shape
    N = w.shape[0]
    y = out if out is not None else torch.empty((M, N // 2 if glu else N), dtype=x2.dtype, device=x2.device)
    epi = (EPI_BIAS if bias is not None else 0) | (EPI_RESID if residual is not None else 0) | (EPI_GLU if glu else 0)
    epi |= {"gelu": EPI_GELU, "relu": EPI_RELU, "silu": EPI_SILU}.get(act or "", 0)
    b = None if bias is None else bias.to(w.dtype).contiguous()
    r = None if residual is None else residual.reshape(M, N).to(x2.dtype)
    if r is not None and r.stride(-1) != 1:
        r = r.contiguous()
    if y.dtype != x2.dtype or y.stride(-1) != 1:
        raise ValueError("gemv: out must be x's dtype with unit inner stride")
    if lora is not None:
        if x2.dtype != torch.float32 or w.dtype != torch.float32:
            raise ValueError("gemv: the adapter epilogue takes fp32 x and W")
        _lib.check(_lib.lib().nos_gemv_lora(x2.data_ptr(), x2.stride(0), *_parts_args(None), w.data_ptr(), w.stride(0),
                                            _ptr(b), _ptr(r), r.stride(0) if r is not None else 0, y.data_ptr(),
                                            y.stride(0), M, N, K, epi, float(rms_eps), *_lora_args(lora, M, N),
                                            _stream()), "nos_gemv_lora")
        return y
    _lib.check(_lib.lib().nos_gemv(x2.data_ptr(), _bf(x2), x2.stride(0), w.data_ptr(), _bf(w), w.stride(0), _ptr(b),
                                   _ptr(r), r.stride(0) if r is not None else 0, y.data_ptr(), y.stride(0), M, N, K,
                                   epi, float(rms_eps), _stream()), "nos_gemv")
    return y


def linear_lora(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, act: str | None = None,
                residual: torch.Tensor | None = None, lora: tuple | None = None) -> torch.Tensor:
    """act(x @ W^T + B[sel] @ t + b) + R for fp32 decode rows x [..., K]: :func:`gemv` with the adapter
    epilogue.  Rows the GEMV does not take are an error (the adapter epilogue exists nowhere else)."""
    K, N = x.shape[-1], w.shape[0]
    x2 = x.reshape(-1, K)
    if x2.stride(-1) != 1 or x2.stride(0) % 4 or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    if not gemv_ok(x2, w) or x2.dtype != torch.float32 or w.dtype != torch.float32:
        raise ValueError(f"linear_lora: x {tuple(x.shape)} {x.dtype} and W {tuple(w.shape)} {w.dtype} are not a product "
                         f"the fp32 GEMV takes (gemv_ok)")
    return gemv(x2, w, bias, act, residual, lora=lora).view(*x.shape[:-1], N)


def lora(x: torch.Tensor, A: torch.Tensor, B: torch.Tensor, sel: torch.Tensor) -> torch.Tensor:
    """``lora(x, A, B, sel)`` (:func:`lora_ref`) of fp32 x [batch, S, K] on the device, for steps of more
    rows than the GEMVs take (a prefill): each sequence's A and B gathered by ``index_select`` on
    ``sel``, two ``bmm`` and a mask for the base rows -- stream-ordered, no host read of ``sel``.  CPU
    tensors: the reference."""
    if not x.is_cuda:
        return lora_ref(x, A, B, sel)
    ok, idx = _lora_rows(sel, A.shape[0], x.shape[0], 1)
    t = torch.bmm(x, A.index_select(0, idx).transpose(1, 2))
    y = torch.bmm(t, B.index_select(0, idx).transpose(1, 2))
    return y * ok.view(-1, 1, 1).to(y.dtype)


def gemv_partials(p: DecodePartials, w: torch.Tensor, bias: torch.Tensor | None = None, act: str | None = None,
                  residual: torch.Tensor | None = None, lora: tuple | None = None) -> torch.Tensor:
    """:func:`gemv` whose x [B, H x D] is the decode attention's output,
    combined from its split partials in the kernel's x staging
    (decode.hip ``parts_x4``, the combine kernel's arithmetic): y [B, N] fp32."""
    B, _, H, D = p.shape
    K = H * D
    N = w.shape[0]
    if w.shape[1] != K or w.stride(-1) != 1 or w.stride(0) % 4 or w.data_ptr() % 16 or B > GEMV_MAX_ROWS:
        raise ValueError(f"gemv_partials: W {tuple(w.shape)} for x [{B}, {K}]")
    y = torch.empty((B, N), dtype=torch.float32, device=w.device)
    epi = (EPI_BIAS if bias is not None else 0) | (EPI_RESID if residual is not None else 0)
    epi |= {"gelu": EPI_GELU, "relu": EPI_RELU, "silu": EPI_SILU}.get(act or "", 0)
    b = None if bias is None else bias.to(w.dtype).contiguous()
    r = None if residual is None else residual.reshape(B, N).float()
    if r is not None and r.stride(-1) != 1:
        r = r.contiguous()
    if lora is not None:   # the adapter epilogue (as gemv's), fp32 W
        if w.dtype != torch.float32:
            raise ValueError("gemv_partials: the adapter epilogue takes an fp32 W")
        _lib.check(_lib.lib().nos_gemv_lora(None, K, *_parts_args(p), w.data_ptr(), w.stride(0), _ptr(b), _ptr(r),
                                            r.stride(0) if r is not None else 0, y.data_ptr(), y.stride(0), B, N, K,
                                            epi, 0.0, *_lora_args(lora, B, N), _stream()), "nos_gemv_lora")
        return y
    _lib.check(_lib.lib().nos_gemv_partials(p.ws.data_ptr(), p.ws.numel(), p.NS, p.G, p.G, p.Hkv, D, 0, w.data_ptr(),
                                            _bf(w), w.stride(0), _ptr(b), _ptr(r), r.stride(0) if r is not None else 0,
                                            y.data_ptr(), y.stride(0), B, N, K, epi, _stream()), "nos_gemv_partials")
    return y


# ------------------------------------------------------------------ int8 weight-only linears
def _q8_epi(bias, act, residual, glu) -> int:
    epi = (EPI_BIAS if bias is not None else 0) | (EPI_RESID if residual is not None else 0) | (EPI_GLU if glu else 0)
    return epi | {"gelu": EPI_GELU, "relu": EPI_RELU, "silu": EPI_SILU}.get(act or "", 0)


def linear_q8_ref(x, wq, wscale, bias=None, act=None, residual=None, rms_eps: float = 0.0, gamma=None,
                  glu: bool = False, dtype: torch.dtype = torch.float32, lora: tuple | None = None):
    """What an int8 weight-only linear means, in ``dtype`` arithmetic:
    ``act(x' @ (wq.float() * wscale[:, None]).T + bias) + residual`` with
    ``x' = rmsnorm(x) * gamma`` when ``rms_eps`` > 0, ``silu(gate) * up`` of
    the two halves of the columns for ``glu``.  The dequantized weight is
    formed in fp32 (one rounding, the storage format's definition) whatever
    ``dtype`` the product runs in."""
    wf = (wq.to(torch.float32) * wscale.to(torch.float32)[:, None]).to(dtype)
    xf = x.to(dtype)
    if rms_eps:
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + rms_eps)
        if gamma is not None:
            xf = xf * gamma.to(dtype)
    y = F.linear(xf, wf, None if bias is None else bias.to(dtype))
    if lora is not None:   # (t, B, sel, rows_per_seq): the adapter delta joins the product before the bias
        y = y + lora_expand_ref(lora[0], lora[1], lora[2], lora[3], dtype).reshape(y.shape)
    if glu:
        h = y.shape[-1] // 2
        y = F.silu(y[..., :h]) * y[..., h:]
    y = F.silu(y) if act == "silu" else _act(y, act)
    return y if residual is None else y + residual.to(dtype).reshape(y.shape)


def gemv_q8_ok(x2: torch.Tensor, wq: torch.Tensor) -> bool:
    """Whether the int8 GEMV takes this [M, K] fp32 x [N, K] int8 product."""
    M, K = x2.shape
    return (x2.is_cuda and 0 < M <= GEMV_MAX_ROWS and K % 16 == 0 and M * K * 4 <= 65536 and x2.stride(-1) == 1
            and x2.stride(0) % 4 == 0 and x2.dtype == torch.float32 and x2.data_ptr() % 16 == 0
            and wq.dtype == torch.int8 and wq.dim() == 2 and wq.shape[1] == K and wq.stride(-1) == 1
            and wq.stride(0) % 16 == 0 and wq.data_ptr() % 16 == 0)


def _q8_operands(wscale, gamma, bias, residual, M, N, K=None):
    if (wscale.numel() != N or (bias is not None and bias.numel() != N) or (gamma is not None and gamma.numel() != K)
            or (residual is not None and residual.numel() != M * N)):
        raise ValueError(f"linear_q8: wscale / bias [{N}], gamma [{K}] and residual [{M}, {N}] required")
    sc = wscale.float().contiguous()
    g = None if gamma is None else gamma.float().contiguous()
    b = None if bias is None else bias.float().contiguous()
    r = None if residual is None else residual.reshape(M, N).float()
    if r is not None and r.stride(-1) != 1:
        r = r.contiguous()
    return sc, g, b, r


def gemv_q8(x2: torch.Tensor, wq: torch.Tensor, wscale: torch.Tensor, bias: torch.Tensor | None = None,
            act: str | None = None, residual: torch.Tensor | None = None, rms_eps: float = 0.0,
            gamma: torch.Tensor | None = None, glu: bool = False, lora: tuple | None = None) -> torch.Tensor:
    """y [M, N] = act(x' [M, K] (wq * wscale)^T + b) + R for M <= 8
    (:func:`gemv_q8_ok`; :func:`linear_q8_ref` defines x' and ``glu``): the
    weight-streaming kernel of an int8 tenant's decode step, one byte of HBM
    per weight, fp32 FMAs on the int8 values and the row scale in the epilogue."""
    M, K = x2.shape
    N = wq.shape[0]
    y = torch.empty((M, N // 2 if glu else N), dtype=torch.float32, device=x2.device)
    if not gemv_q8_ok(x2, wq) or (glu and N % 2):
        raise ValueError(f"gemv_q8: x {tuple(x2.shape)} {x2.dtype} and W {tuple(wq.shape)} {wq.dtype} are not a "
                         f"product the int8 GEMV takes (gemv_q8_ok)")
    sc, g, b, r = _q8_operands(wscale, gamma, bias, residual, M, N, K)
    if lora is not None:   # the adapter epilogue (as gemv's)
        _lib.check(_lib.lib().nos_gemv_q8_lora(x2.data_ptr(), x2.stride(0), *_parts_args(None), wq.data_ptr(),
                                               wq.stride(0), sc.data_ptr(), _ptr(g), _ptr(b), _ptr(r),
                                               r.stride(0) if r is not None else 0, y.data_ptr(), y.stride(0), M, N, K,
                                               _q8_epi(b, act, r, glu), float(rms_eps), *_lora_args(lora, M, N),
                                               _stream()), "nos_gemv_q8_lora")
        return y
    _lib.check(_lib.lib().nos_gemv_q8(x2.data_ptr(), x2.stride(0), wq.data_ptr(), wq.stride(0), sc.data_ptr(), _ptr(g),
                                      _ptr(b), _ptr(r), r.stride(0) if r is not None else 0, y.data_ptr(), y.stride(0),
                                      M, N, K, _q8_epi(b, act, r, glu), float(rms_eps), _stream()), "nos_gemv_q8")
    return y


def gemv_q8_partials(p: DecodePartials, wq: torch.Tensor, wscale: torch.Tensor, bias: torch.Tensor | None = None,
                     act: str | None = None, residual: torch.Tensor | None = None,
                     lora: tuple | None = None) -> torch.Tensor:
    """:func:`gemv_q8` whose x [B, H x D] is the decode attention's output,
    combined from its split partials in the kernel's x staging (as
    :func:`gemv_partials`): y [B, N] fp32."""
    B, _, H, D = p.shape
    K = H * D
    N = wq.shape[0]
    if (wq.dtype != torch.int8 or wq.shape[1] != K or wq.stride(-1) != 1 or wq.stride(0) % 16 or wq.data_ptr() % 16
            or B > GEMV_MAX_ROWS):
        raise ValueError(f"gemv_q8_partials: W {tuple(wq.shape)} {wq.dtype} for x [{B}, {K}]")
    y = torch.empty((B, N), dtype=torch.float32, device=wq.device)
    sc, _, b, r = _q8_operands(wscale, None, bias, residual, B, N)
    if lora is not None:   # the adapter epilogue (as gemv's)
        _lib.check(_lib.lib().nos_gemv_q8_lora(None, K, *_parts_args(p), wq.data_ptr(), wq.stride(0), sc.data_ptr(), None,
                                               _ptr(b), _ptr(r), r.stride(0) if r is not None else 0, y.data_ptr(),
                                               y.stride(0), B, N, K, _q8_epi(b, act, r, False), 0.0,
                                               *_lora_args(lora, B, N), _stream()), "nos_gemv_q8_lora")
        return y
    _lib.check(_lib.lib().nos_gemv_q8_partials(p.ws.data_ptr(), p.ws.numel(), p.NS, p.G, p.G, p.Hkv, D, wq.data_ptr(),
                                               wq.stride(0), sc.data_ptr(), _ptr(b), _ptr(r),
                                               r.stride(0) if r is not None else 0, y.data_ptr(), y.stride(0), B, N, K,
                                               _q8_epi(b, act, r, False), _stream()), "nos_gemv_q8_partials")
    return y


def dequant_q8(wq: torch.Tensor, wscale: torch.Tensor) -> torch.Tensor:
    """``wq.float() * wscale[:, None]`` as a fresh fp32 [N, K] tensor, bit for bit."""
    if not wq.is_cuda:
        return wq.to(torch.float32) * wscale.to(torch.float32)[:, None]
    N, K = wq.shape
    if wq.dtype != torch.int8 or wq.stride(-1) != 1 or K % 4 or wq.stride(0) % 4 or wq.data_ptr() % 4:
        raise ValueError(f"dequant_q8: an int8 [N, K] weight with K % 4 == 0 and 4-byte aligned rows, got "
                         f"{tuple(wq.shape)} {wq.dtype}")
    out = torch.empty((N, K), dtype=torch.float32, device=wq.device)
    sc = wscale.float().contiguous()
    _lib.check(_lib.lib().nos_dequant_q8(wq.data_ptr(), wq.stride(0), sc.data_ptr(), out.data_ptr(), K, N, K,
                                         _stream()), "nos_dequant_q8")
    return out


def linear_q8(x: torch.Tensor, wq: torch.Tensor, wscale: torch.Tensor, bias: torch.Tensor | None = None,
              act: str | None = None, residual: torch.Tensor | None = None, rms_eps: float = 0.0,
              gamma: torch.Tensor | None = None, glu: bool = False, lora: tuple | None = None) -> torch.Tensor:
    """The int8 weight-only linear (:func:`linear_q8_ref`) of fp32 x [..., K]:
    at most :data:`GEMV_MAX_ROWS` rows on :func:`gemv_q8`; more rows
    dequantize the weight into a transient fp32 buffer (freed with the
    call's other intermediates, never cached) for the run-time-split h3
    product, after the ``rmsnorm`` kernel when there is a prologue.  CPU
    tensors: the reference.  ``lora``: the adapter operand of :func:`gemv` -- on the GPU for rows the
    int8 GEMV takes only (an error otherwise)."""
    if not x.is_cuda:
        return linear_q8_ref(x, wq, wscale, bias, act, residual, rms_eps, gamma, glu, lora=lora)
    if x.dtype != torch.float32:
        raise ValueError(f"linear_q8 takes an fp32 x, got {x.dtype}")
    K, N = x.shape[-1], wq.shape[0]
    x2 = x.reshape(-1, K)
    if x2.stride(-1) != 1 or x2.stride(0) % 4 or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.shape[0]
    shape = (*x.shape[:-1], N // 2 if glu else N)
    if M <= GEMV_MAX_ROWS and gemv_q8_ok(x2, wq):
        return gemv_q8(x2, wq, wscale, bias, act, residual, rms_eps, gamma, glu, lora=lora).view(shape)
    if lora is not None:
        raise ValueError(f"linear_q8: the adapter epilogue exists on the int8 GEMV only; x {tuple(x.shape)} and W "
                         f"{tuple(wq.shape)} are not a product it takes (gemv_q8_ok)")
    if rms_eps:
        x2 = rmsnorm(x2, gamma if gamma is not None else torch.ones(K, dtype=torch.float32, device=x.device), rms_eps)
    r = None if residual is None else residual.reshape(M, N).float().contiguous()
    gemm_act = act if act in ("gelu", "relu") else None   # the GEMM's epilogue; silu: a pass of its own
    y = mm(x2, dequant_q8(wq, wscale), b_t=True, bias=bias, act=gemm_act, residual=r if act == gemm_act else None)
    if glu:
        return _glu_halves(y).view(shape)
    if act != gemm_act:
        y = unary(y, act, torch.float32)
        if r is not None:
            y = y + r
    return y.view(shape)


# ------------------------------------------------------------------ MXFP4 weight-only linears
MX4_BLOCK = 32   # consecutive k of a row under one E8M0 scale byte (podserver.program.builder.quantize_rows_mx4)
_MX4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)


def _mx4_weight_ok(wq: torch.Tensor, wscale: torch.Tensor) -> bool:
    return (wq.dtype == torch.uint8 and wscale.dtype == torch.uint8 and wq.dim() == 2 and wscale.dim() == 2
            and wq.shape[0] == wscale.shape[0] and wq.shape[1] * 2 == wscale.shape[1] * MX4_BLOCK)


def _dequant_mx4_ref(wq: torch.Tensor, wscale: torch.Tensor) -> torch.Tensor:
    """``builder.dequantize_rows_mx4`` in torch: fp32 [N, K] = elem x 2^(e - 127), exact."""
    if not _mx4_weight_ok(wq, wscale):
        raise ValueError(f"an MXFP4 weight is codes u8 [N, K / 2] and scales u8 [N, K / {MX4_BLOCK}], got "
                         f"{tuple(wq.shape)} {wq.dtype} and {tuple(wscale.shape)} {wscale.dtype}")
    table = torch.tensor(_MX4_VALUES, dtype=torch.float32, device=wq.device)
    idx = torch.stack(((wq & 15).long(), (wq >> 4).long()), dim=-1).reshape(wq.shape[0], -1)
    e = wscale.to(torch.int32).repeat_interleave(MX4_BLOCK, dim=1) - 127
    return torch.ldexp(table[idx], e)


def linear_mx4_ref(x, wq, wscale, bias=None, act=None, residual=None, rms_eps: float = 0.0, gamma=None,
                   glu: bool = False, dtype: torch.dtype = torch.float32):
    """What an MXFP4 weight-only linear means, in ``dtype`` arithmetic:
    ``act(x' @ W.T + bias) + residual`` with W = ``dequantize_rows_mx4(wq, wscale)`` formed in fp32
    (exact: the storage format's definition), ``x' = rmsnorm(x) * gamma`` when ``rms_eps`` > 0 and
    ``silu(gate) * up`` of the two halves of the columns for ``glu``."""
    wf = _dequant_mx4_ref(wq, wscale).to(dtype)
    xf = x.to(dtype)
    if rms_eps:
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + rms_eps)
        if gamma is not None:
            xf = xf * gamma.to(dtype)
    y = F.linear(xf, wf, None if bias is None else bias.to(dtype))
    if glu:
        h = y.shape[-1] // 2
        y = F.silu(y[..., :h]) * y[..., h:]
    y = F.silu(y) if act == "silu" else _act(y, act)
    return y if residual is None else y + residual.to(dtype).reshape(y.shape)


def gemv_mx4_ok(x2: torch.Tensor, wq: torch.Tensor) -> bool:
    """Whether the MXFP4 GEMV takes this [M, K] fp32 x [N, K / 2] u8 product."""
    M, K = x2.shape
    return (x2.is_cuda and 0 < M <= GEMV_MAX_ROWS and K % MX4_BLOCK == 0 and M * K * 4 <= GEMV_X_BYTES
            and x2.stride(-1) == 1 and x2.stride(0) % 4 == 0 and x2.dtype == torch.float32 and x2.data_ptr() % 16 == 0
            and wq.dtype == torch.uint8 and wq.dim() == 2 and wq.shape[1] * 2 == K and wq.stride(-1) == 1
            and wq.stride(0) % 16 == 0 and wq.data_ptr() % 16 == 0)


def _mx4_operands(wq, wscale, gamma, bias, residual, M, N, K):
    if (not _mx4_weight_ok(wq, wscale) or wq.shape[1] * 2 != K or (bias is not None and bias.numel() != N)
            or (gamma is not None and gamma.numel() != K) or (residual is not None and residual.numel() != M * N)):
        raise ValueError(f"linear_mx4: codes u8 [{N}, {K // 2}], wscale u8 [{N}, {K // MX4_BLOCK}], bias [{N}], gamma "
                         f"[{K}] and residual [{M}, {N}] required")
    sc = wscale if wscale.stride(-1) == 1 else wscale.contiguous()
    g = None if gamma is None else gamma.float().contiguous()
    b = None if bias is None else bias.float().contiguous()
    r = None if residual is None else residual.reshape(M, N).float()
    if r is not None and r.stride(-1) != 1:
        r = r.contiguous()
    return sc, g, b, r


def gemv_mx4(x2: torch.Tensor, wq: torch.Tensor, wscale: torch.Tensor, bias: torch.Tensor | None = None,
             act: str | None = None, residual: torch.Tensor | None = None, rms_eps: float = 0.0,
             gamma: torch.Tensor | None = None, glu: bool = False) -> torch.Tensor:
    """y [M, N] = act(x' [M, K] W^T + b) + R for M <= 8 (:func:`gemv_mx4_ok`;
    :func:`linear_mx4_ref` defines W, x' and ``glu``): the weight-streaming kernel of an MXFP4 tenant's
    decode step, 4.25 bits of HBM per weight, fp32 FMAs on the dequantized values.  Every scale byte
    must lie in [2, 252] (a registration checks it; this call does not read them)."""
    M, K = x2.shape
    N = wq.shape[0]
    if not gemv_mx4_ok(x2, wq) or (glu and N % 2):
        raise ValueError(f"gemv_mx4: x {tuple(x2.shape)} {x2.dtype} and codes {tuple(wq.shape)} {wq.dtype} are not a "
                         f"product the MXFP4 GEMV takes (gemv_mx4_ok)")
    sc, g, b, r = _mx4_operands(wq, wscale, gamma, bias, residual, M, N, K)
    y = torch.empty((M, N // 2 if glu else N), dtype=torch.float32, device=x2.device)
    _lib.check(_lib.lib().nos_gemv_mx4(x2.data_ptr(), x2.stride(0), wq.data_ptr(), wq.stride(0), sc.data_ptr(),
                                       sc.stride(0), _ptr(g), _ptr(b), _ptr(r), r.stride(0) if r is not None else 0,
                                       y.data_ptr(), y.stride(0), M, N, K, _q8_epi(b, act, r, glu), float(rms_eps),
                                       _stream()), "nos_gemv_mx4")
    return y


def gemv_mx4_partials(p: DecodePartials, wq: torch.Tensor, wscale: torch.Tensor, bias: torch.Tensor | None = None,
                      act: str | None = None, residual: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`gemv_mx4` whose x [B, H x D] is the decode attention's output, combined from its split
    partials in the kernel's x staging (as :func:`gemv_partials`): y [B, N] fp32."""
    B, _, H, D = p.shape
    K = H * D
    N = wq.shape[0]
    if (wq.dtype != torch.uint8 or wq.dim() != 2 or wq.shape[1] * 2 != K or wq.stride(-1) != 1 or wq.stride(0) % 16
            or wq.data_ptr() % 16 or B > GEMV_MAX_ROWS):
        raise ValueError(f"gemv_mx4_partials: codes {tuple(wq.shape)} {wq.dtype} for x [{B}, {K}]")
    sc, _, b, r = _mx4_operands(wq, wscale, None, bias, residual, B, N, K)
    y = torch.empty((B, N), dtype=torch.float32, device=wq.device)
    _lib.check(_lib.lib().nos_gemv_mx4_partials(p.ws.data_ptr(), p.ws.numel(), p.NS, p.G, p.G, p.Hkv, D, wq.data_ptr(),
                                                wq.stride(0), sc.data_ptr(), sc.stride(0), _ptr(b), _ptr(r),
                                                r.stride(0) if r is not None else 0, y.data_ptr(), y.stride(0), B, N, K,
                                                _q8_epi(b, act, r, False), _stream()), "nos_gemv_mx4_partials")
    return y


def dequant_mx4(wq: torch.Tensor, wscale: torch.Tensor) -> torch.Tensor:
    """``dequantize_rows_mx4(wq, wscale)`` as a fresh fp32 [N, K] tensor, bit for bit (scale bytes in
    [2, 252]); on the GPU by the GEMV's own conversion (decode.hip ``nos_dequant_mx4``)."""
    if not wq.is_cuda:
        return _dequant_mx4_ref(wq, wscale)
    if not _mx4_weight_ok(wq, wscale) or wq.stride(-1) != 1 or wq.stride(0) % 4 or wq.data_ptr() % 4:
        raise ValueError(f"dequant_mx4: codes u8 [N, K / 2] with 4-byte aligned rows and scales u8 [N, K / {MX4_BLOCK}], "
                         f"got {tuple(wq.shape)} {wq.dtype} and {tuple(wscale.shape)} {wscale.dtype}")
    N, K = wq.shape[0], wq.shape[1] * 2
    out = torch.empty((N, K), dtype=torch.float32, device=wq.device)
    sc = wscale if wscale.stride(-1) == 1 else wscale.contiguous()
    _lib.check(_lib.lib().nos_dequant_mx4(wq.data_ptr(), wq.stride(0), sc.data_ptr(), sc.stride(0), out.data_ptr(), K,
                                          N, K, _stream()), "nos_dequant_mx4")
    return out


def linear_mx4(x: torch.Tensor, wq: torch.Tensor, wscale: torch.Tensor, bias: torch.Tensor | None = None,
               act: str | None = None, residual: torch.Tensor | None = None, rms_eps: float = 0.0,
               gamma: torch.Tensor | None = None, glu: bool = False) -> torch.Tensor:
    """The MXFP4 weight-only linear (:func:`linear_mx4_ref`) of fp32 x [..., K]: at most
    :data:`GEMV_MAX_ROWS` rows that fit :data:`GEMV_X_BYTES` on :func:`gemv_mx4`; otherwise the weight
    is dequantized into a transient fp32 buffer (freed with the call's other intermediates, never
    cached) for the run-time-split h3 product, after the ``rmsnorm`` kernel when there is a prologue.
    CPU tensors: the reference."""
    if not x.is_cuda:
        return linear_mx4_ref(x, wq, wscale, bias, act, residual, rms_eps, gamma, glu)
    if x.dtype != torch.float32:
        raise ValueError(f"linear_mx4 takes an fp32 x, got {x.dtype}")
    K, N = x.shape[-1], wq.shape[0]
    x2 = x.reshape(-1, K)
    if x2.stride(-1) != 1 or x2.stride(0) % 4 or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = x2.shape[0]
    shape = (*x.shape[:-1], N // 2 if glu else N)
    if M <= GEMV_MAX_ROWS and gemv_mx4_ok(x2, wq):
        return gemv_mx4(x2, wq, wscale, bias, act, residual, rms_eps, gamma, glu).view(shape)
    if rms_eps:
        x2 = rmsnorm(x2, gamma if gamma is not None else torch.ones(K, dtype=torch.float32, device=x.device), rms_eps)
    r = None if residual is None else residual.reshape(M, N).float().contiguous()
    gemm_act = act if act in ("gelu", "relu") else None   # the GEMM's epilogue; silu: a pass of its own
    y = mm(x2, dequant_mx4(wq, wscale), b_t=True, bias=bias, act=gemm_act, residual=r if act == gemm_act else None)
    if glu:
        return _glu_halves(y).view(shape)
    if act != gemm_act:
        y = unary(y, act, torch.float32)
        if r is not None:
            y = y + r
    return y.view(shape)


def _glu_halves(y: torch.Tensor) -> torch.Tensor:
    """silu(gate) * up of the two column halves of a merged [gate; up] product."""
    h = y.shape[-1] // 2
    return glu(y[..., :h], y[..., h:], "silu")


# ------------------------------------------------------------------ mixture of experts
MOE_MAX_EXPERTS = 64   # a lane per expert in the route kernel (decode.hip MOE_MAX_E)
MOE_MAX_TOP_K = 8      # decode.hip MOE_MAX_K


def _moe_x(x2, rms_eps, gamma, dtype):
    """x' of the MoE kernels in ``dtype``: x, RMS-normalised and times ``gamma`` when ``rms_eps`` > 0."""
    xf = x2.to(dtype)
    if rms_eps:
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + rms_eps)
        if gamma is not None:
            xf = xf * gamma.to(dtype)
    return xf


def _moe_slots(idx, E: int):
    """Per slot of idx [rows, k]: (its expert lies in [0, E)?, the index clamped into it); no host read."""
    e = idx.to(torch.long)
    return (e >= 0) & (e < E), e.clamp(0, E - 1)


def moe_route_ref(x2, Wr, k: int, rms_eps: float = 0.0, gamma=None, dtype: torch.dtype = torch.float32):
    """:func:`moe_route` in ``dtype`` arithmetic: p = softmax(Wr x') over all E experts, the k largest
    by k rounds of arg-max (a tie goes to the lower index) as idx [rows, k] i32 in descending order of
    p, and w = p[idx] / sum(p[idx])."""
    p = torch.softmax(_moe_x(x2, rms_eps, gamma, dtype) @ Wr.to(dtype).T, dim=-1)
    cand, picks = p.clone(), []
    for _ in range(int(k)):
        i = cand.argmax(dim=-1, keepdim=True)   # the first maximal value: the lower index
        picks.append(i)
        cand.scatter_(1, i, -1.0)
    idx = torch.cat(picks, dim=1)
    ps = p.gather(1, idx)
    tot = ps[:, 0].clone()
    for s in range(1, int(k)):   # in slot order
        tot = tot + ps[:, s]
    return idx.to(torch.int32), ps / tot[:, None]


def moe_glu_ref(x2, idx, W13, rms_eps: float = 0.0, gamma=None, dtype: torch.dtype = torch.float32):
    """:func:`moe_glu` in ``dtype`` arithmetic: act [rows, k, I], ``act[m, s] = silu(W13[e][:I] x'[m]) *
    (W13[e][I:] x'[m])`` for e = idx[m, s]; zeros for an e outside [0, E)."""
    rows, k = idx.shape
    I = W13.shape[1] // 2
    ok, e = _moe_slots(idx, W13.shape[0])
    xf = _moe_x(x2, rms_eps, gamma, dtype).repeat_interleave(k, dim=0)
    gu = torch.bmm(W13.index_select(0, e.reshape(-1)).to(dtype), xf.unsqueeze(-1)).squeeze(-1)
    act = (F.silu(gu[:, :I]) * gu[:, I:]).view(rows, k, I)
    return torch.where(ok.unsqueeze(-1), act, torch.zeros_like(act))


def moe_down_ref(act, idx, w, W2, res=None, dtype: torch.dtype = torch.float32):
    """:func:`moe_down` in ``dtype`` arithmetic: ``y[m] = res[m] + sum_s w[m, s] * (W2[idx[m, s]] @ act[m, s])``,
    the slots summed in the order 0 .. k - 1; a slot whose index is outside [0, E) contributes zero."""
    rows, k, I = act.shape
    ok, e = _moe_slots(idx, W2.shape[0])
    d = torch.bmm(W2.index_select(0, e.reshape(-1)).to(dtype), act.to(dtype).reshape(rows * k, I, 1)).view(rows, k, -1)
    d = torch.where(ok.unsqueeze(-1), w.to(dtype).unsqueeze(-1) * d, torch.zeros_like(d))
    y = d[:, 0]
    for s in range(1, k):
        y = y + d[:, s]
    return y if res is None else res.to(dtype).reshape(rows, -1) + y


def moe_ref(x, Wr, W13, W2, k: int, dtype: torch.dtype | None = None):
    """What ``moe(x, Wr, W13, W2; top_k=k)`` means (transformers' ``MixtralSparseMoeBlock``), in ``dtype``
    arithmetic (default: x's): per row of x [..., H], p = softmax(Wr x) over the E experts, the k
    largest (a tie: the lower index) renormalised to sum 1, and ``y = sum_s w_s W2[e_s] (silu(W13[e_s][:I]
    x) * (W13[e_s][I:] x))`` in descending order of p.  Wr [E, H], W13 [E, 2I, H] (gate rows, then up
    rows), W2 [E, H, I]."""
    dt = dtype or x.dtype
    x2 = x.reshape(-1, x.shape[-1])
    idx, w = moe_route_ref(x2, Wr, k, dtype=dt)
    y = moe_down_ref(moe_glu_ref(x2, idx, W13, dtype=dt), idx, w, W2, dtype=dt)
    return y.view(x.shape)


def _moe_refuse(what: str, **tensors) -> None:
    """fp32, unit inner stride, 16-byte base and rows: what the MoE kernels load 16 bytes at a time."""
    for name, t in tensors.items():
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be fp32, got {t.dtype}")
        if not t.is_cuda:
            raise ValueError(f"{what}: {name} must be on the GPU with x, it is on {t.device}")
        if t.stride(-1) != 1 or any(s % 4 for s in t.stride()[:-1]) or t.data_ptr() % 16:
            raise ValueError(f"{what}: {name} {tuple(t.shape)} with strides {t.stride()} at offset "
                             f"{t.data_ptr() % 16} of a 16-byte line: unit inner stride, outer strides that are "
                             f"multiples of 4 and a 16-byte aligned base required")


def _moe_dims(what: str, rows: int, E: int, H: int, I: int, k: int) -> None:
    if not (isinstance(k, int) and 1 <= k <= min(E, MOE_MAX_TOP_K)):
        raise ValueError(f"{what}: top_k must be in [1, min(E, {MOE_MAX_TOP_K})] = [1, {min(E, MOE_MAX_TOP_K)}], got {k!r}")
    if E > MOE_MAX_EXPERTS:
        raise ValueError(f"{what}: E = {E} experts, at most {MOE_MAX_EXPERTS}")
    if H % 4 or I % 4:
        raise ValueError(f"{what}: H = {H} and I = {I} must be multiples of 4 (16-byte loads)")
    if not 1 <= rows <= GEMV_MAX_ROWS:
        raise ValueError(f"{what}: {rows} rows; the kernels take 1 .. {GEMV_MAX_ROWS} (GEMV_MAX_ROWS)")
    if H * 4 > GEMV_X_BYTES or k * I * 4 > GEMV_X_BYTES:
        raise ValueError(f"{what}: a row of H = {H} or k x I = {k} x {I} floats is over the {GEMV_X_BYTES} bytes "
                         f"the kernels stage")


def _moe_gamma(what: str, gamma, rms_eps: float, H: int) -> None:
    if gamma is not None and (not rms_eps or gamma.dim() != 1 or gamma.shape[0] != H):
        raise ValueError(f"{what}: gamma must be [{H}] and comes with rms_eps > 0 only")


def _moe_idx(what: str, idx, rows: int, k: int | None = None) -> None:
    if (idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != rows or not idx.is_contiguous()
            or (k is not None and idx.shape[1] != k) or not idx.is_cuda):
        raise ValueError(f"{what}: idx must be a contiguous i32 [{rows}, k] on the GPU, got {idx.dtype} "
                         f"{tuple(idx.shape)} on {idx.device}")


def moe_route(x: torch.Tensor, Wr: torch.Tensor, k: int, rms_eps: float = 0.0, gamma: torch.Tensor | None = None,
              out: tuple | None = None):
    """(idx [rows, k] i32, w [rows, k] fp32) of x [rows <= 8, H] fp32 and the router Wr [E <= 64, H]: the
    k experts of each row in descending order of p = softmax(Wr x') and their renormalised weights
    (decode.hip ``nos_moe_route``; x' is x under the RMSNorm prologue ``rms_eps`` > 0, ``gamma``).  A
    tie goes to the lower index.  ``out``: contiguous (idx, w) destinations.  CPU tensors:
    :func:`moe_route_ref`."""
    if x.dim() != 2 or Wr.dim() != 2 or Wr.shape[1] != x.shape[1]:
        raise ValueError(f"moe_route: x [rows, H] and Wr [E, H] required, got {tuple(x.shape)} and {tuple(Wr.shape)}")
    rows, H = x.shape
    _moe_gamma("moe_route", gamma, rms_eps, H)
    if not x.is_cuda:
        return moe_route_ref(x, Wr, k, rms_eps, gamma)
    _moe_dims("moe_route", rows, Wr.shape[0], H, 4, k)
    _moe_refuse("moe_route", x=x, Wr=Wr, gamma=gamma)
    if out is not None:
        idx, w = out
        _moe_idx("moe_route", idx, rows, k)
        if w.dtype != torch.float32 or tuple(w.shape) != (rows, k) or not w.is_contiguous() or not w.is_cuda:
            raise ValueError(f"moe_route: out w must be a contiguous fp32 [{rows}, {k}] on the GPU, got {w.dtype} "
                             f"{tuple(w.shape)} on {w.device}")
    else:
        idx = torch.empty((rows, k), dtype=torch.int32, device=x.device)
        w = torch.empty((rows, k), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().nos_moe_route(x.data_ptr(), x.stride(0), Wr.data_ptr(), Wr.stride(0), _ptr(gamma),
                                        float(rms_eps), idx.data_ptr(), w.data_ptr(), rows, Wr.shape[0], H, int(k),
                                        _stream()), "nos_moe_route")
    return idx, w


def moe_glu(x: torch.Tensor, idx: torch.Tensor, W13: torch.Tensor, rms_eps: float = 0.0,
            gamma: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """act [rows, k, I] fp32: ``silu(W13[e][:I] x'[m]) * (W13[e][I:] x'[m])`` for e = idx[m, s], of x
    [rows <= 8, H] fp32 and W13 [E, 2I, H] (decode.hip ``nos_moe_glu``; x' as :func:`moe_route`).  The
    kernel checks every index: a slot outside [0, E) reads no weight and is zeros.  ``out``: a
    contiguous destination.  CPU tensors: :func:`moe_glu_ref`."""
    if x.dim() != 2 or W13.dim() != 3 or W13.shape[2] != x.shape[1] or W13.shape[1] % 2 or idx.dim() != 2:
        raise ValueError(f"moe_glu: x [rows, H], idx [rows, k] and W13 [E, 2I, H] required, got {tuple(x.shape)}, "
                         f"{tuple(idx.shape)} and {tuple(W13.shape)}")
    rows, H = x.shape
    _moe_gamma("moe_glu", gamma, rms_eps, H)
    if not x.is_cuda:
        return moe_glu_ref(x, idx, W13, rms_eps, gamma)
    E, I, k = W13.shape[0], W13.shape[1] // 2, idx.shape[1]
    _moe_dims("moe_glu", rows, E, H, I, k)
    _moe_idx("moe_glu", idx, rows)
    _moe_refuse("moe_glu", x=x, W13=W13, gamma=gamma)
    act = out if out is not None else torch.empty((rows, k, I), dtype=torch.float32, device=x.device)
    if (act.dtype != torch.float32 or tuple(act.shape) != (rows, k, I) or not act.is_contiguous() or not act.is_cuda
            or act.data_ptr() % 16):
        raise ValueError(f"moe_glu: out must be a contiguous, 16-byte aligned fp32 [{rows}, {k}, {I}] on the GPU, got "
                         f"{act.dtype} {tuple(act.shape)} on {act.device}")
    _lib.check(_lib.lib().nos_moe_glu(x.data_ptr(), x.stride(0), idx.data_ptr(), W13.data_ptr(), W13.stride(0),
                                      W13.stride(1), _ptr(gamma), float(rms_eps), act.data_ptr(), rows, E, H, I, k,
                                      _stream()), "nos_moe_glu")
    return act


def moe_down(act: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, W2: torch.Tensor,
             res: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """y [rows, H] fp32 = ``res + sum_s w[m, s] * (W2[idx[m, s]] @ act[m, s])`` of act [rows <= 8, k, I], w
    [rows, k] and W2 [E, H, I] (decode.hip ``nos_moe_down``), the slots summed in the order 0 .. k - 1
    without atomics: bit-reproducible.  A slot whose index is outside [0, E) contributes zero.  ``out``:
    a [rows, H] destination with unit inner stride.  CPU tensors: :func:`moe_down_ref`."""
    if (act.dim() != 3 or W2.dim() != 3 or W2.shape[2] != act.shape[2] or tuple(w.shape) != tuple(act.shape[:2])
            or tuple(idx.shape) != tuple(act.shape[:2])):
        raise ValueError(f"moe_down: act [rows, k, I], idx and w [rows, k] and W2 [E, H, I] required, got "
                         f"{tuple(act.shape)}, {tuple(idx.shape)}, {tuple(w.shape)} and {tuple(W2.shape)}")
    rows, k, I = act.shape
    E, H = W2.shape[:2]
    if res is not None and tuple(res.shape) != (rows, H):
        raise ValueError(f"moe_down: res must be [{rows}, {H}], got {tuple(res.shape)}")
    if not act.is_cuda:
        y = moe_down_ref(act, idx, w, W2, res)
        return y if out is None else out.copy_(y)
    _moe_dims("moe_down", rows, E, H, I, k)
    _moe_idx("moe_down", idx, rows, k)
    if not act.is_contiguous() or not w.is_contiguous() or w.dtype != torch.float32 or not w.is_cuda:
        raise ValueError(f"moe_down: act and w must be contiguous and w fp32 on the GPU, got w {w.dtype} on {w.device}")
    _moe_refuse("moe_down", act=act, W2=W2)
    y = out if out is not None else torch.empty((rows, H), dtype=torch.float32, device=act.device)
    for name, t in (("res", res), ("out", y)):
        if t is not None and (t.dtype != torch.float32 or not t.is_cuda or t.stride(-1) != 1 or tuple(t.shape) != (rows, H)
                              or t.stride(0) < H):
            raise ValueError(f"moe_down: {name} must be an fp32 [{rows}, {H}] on the GPU with unit inner stride, got "
                             f"{t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    _lib.check(_lib.lib().nos_moe_down(act.data_ptr(), idx.data_ptr(), w.data_ptr(), W2.data_ptr(), W2.stride(0),
                                       W2.stride(1), _ptr(res), res.stride(0) if res is not None else 0, y.data_ptr(),
                                       y.stride(0), rows, E, H, I, k, _stream()), "nos_moe_down")
    return y


def moe(x: torch.Tensor, Wr: torch.Tensor, W13: torch.Tensor, W2: torch.Tensor, k: int) -> torch.Tensor:
    """``moe`` (:func:`moe_ref`) of fp32 x [..., H] on the device for steps of more rows than the kernels
    take (a prefill): PyTorch ops, DENSE over the experts -- every expert's MLP on every row, times a
    gate that is the renormalised p for the k chosen experts (scattered from the arg-max rounds) and 0
    elsewhere; E / k times the useful FLOPs, stream-ordered, no host read of a routing value.  CPU
    tensors: the reference."""
    if not x.is_cuda:
        return moe_ref(x, Wr, W13, W2, k)
    x2 = x.reshape(-1, x.shape[-1])
    idx, w = moe_route_ref(x2, Wr, k)
    gates = torch.zeros((x2.shape[0], Wr.shape[0]), dtype=x2.dtype, device=x.device).scatter_(1, idx.long(), w)
    I = W13.shape[1] // 2
    y = torch.zeros_like(x2)
    for e in range(Wr.shape[0]):
        gu = x2 @ W13[e].T
        y = y + gates[:, e:e + 1] * ((F.silu(gu[:, :I]) * gu[:, I:]) @ W2[e].T)
    return y.view(x.shape)


# ------------------------------------------------------------------ quantized experts (int8, MXFP4)
def _dequant_experts_q8(Wq: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """fp32 [E, N, K] = ``Wq.float() * s[..., None]``, one rounding (``dequantize_rows_q8`` expert by expert)."""
    if Wq.dim() != 3 or tuple(s.shape) != tuple(Wq.shape[:2]):
        raise ValueError(f"int8 experts are codes [E, N, K] and scales [E, N], got {tuple(Wq.shape)} and {tuple(s.shape)}")
    return Wq.to(torch.float32) * s.to(torch.float32).unsqueeze(-1)


def _dequant_experts_mx4(Wc: torch.Tensor, We: torch.Tensor) -> torch.Tensor:
    """fp32 [E, N, K] of MXFP4 experts: codes u8 [E, N, K / 2], scale bytes u8 [E, N, K / 32] (exact)."""
    if Wc.dim() != 3 or We.dim() != 3 or tuple(Wc.shape[:2]) != tuple(We.shape[:2]):
        raise ValueError(f"MXFP4 experts are codes u8 [E, N, K / 2] and scales u8 [E, N, K / {MX4_BLOCK}], got "
                         f"{tuple(Wc.shape)} and {tuple(We.shape)}")
    E, N = Wc.shape[:2]
    return _dequant_mx4_ref(Wc.reshape(E * N, -1), We.reshape(E * N, -1)).view(E, N, -1)


def moe_glu_q8_ref(x2, idx, W13q, s13, rms_eps: float = 0.0, gamma=None, dtype: torch.dtype = torch.float32):
    """:func:`moe_glu_q8` in ``dtype`` arithmetic: :func:`moe_glu_ref` on the experts dequantized in fp32."""
    return moe_glu_ref(x2, idx, _dequant_experts_q8(W13q, s13), rms_eps, gamma, dtype)


def moe_down_q8_ref(act, idx, w, W2q, s2, res=None, dtype: torch.dtype = torch.float32):
    """:func:`moe_down_q8` in ``dtype`` arithmetic: :func:`moe_down_ref` on the experts dequantized in fp32."""
    return moe_down_ref(act, idx, w, _dequant_experts_q8(W2q, s2), res, dtype)


def moe_glu_mx4_ref(x2, idx, W13c, W13e, rms_eps: float = 0.0, gamma=None, dtype: torch.dtype = torch.float32):
    """:func:`moe_glu_mx4` in ``dtype`` arithmetic: :func:`moe_glu_ref` on the dequantized experts."""
    return moe_glu_ref(x2, idx, _dequant_experts_mx4(W13c, W13e), rms_eps, gamma, dtype)


def moe_down_mx4_ref(act, idx, w, W2c, W2e, res=None, dtype: torch.dtype = torch.float32):
    """:func:`moe_down_mx4` in ``dtype`` arithmetic: :func:`moe_down_ref` on the dequantized experts."""
    return moe_down_ref(act, idx, w, _dequant_experts_mx4(W2c, W2e), res, dtype)


def moe_q8_ref(x, Wr, W13q, s13, W2q, s2, k: int, dtype: torch.dtype | None = None):
    """What ``moe_q8(x, Wr, W13q, s13, W2q, s2; top_k=k)`` means: :func:`moe_ref` with the experts
    ``q.float() * scale`` (formed in fp32, the storage format's definition)."""
    return moe_ref(x, Wr, _dequant_experts_q8(W13q, s13), _dequant_experts_q8(W2q, s2), k, dtype)


def moe_mx4_ref(x, Wr, W13c, W13e, W2c, W2e, k: int, dtype: torch.dtype | None = None):
    """What ``moe_mx4(x, Wr, W13c, W13e, W2c, W2e; top_k=k)`` means: :func:`moe_ref` with the experts
    ``elem x 2^(e - 127)`` (exact in fp32)."""
    return moe_ref(x, Wr, _dequant_experts_mx4(W13c, W13e), _dequant_experts_mx4(W2c, W2e), k, dtype)


_MOE_QUANT = {"q8": (16, torch.int8, 1, "int8"), "mx4": (MX4_BLOCK, torch.uint8, 2, "MXFP4")}   # K multiple, codes, k per byte


def _moe_quant_weights(what: str, fmt: str, Wq, S, E: int, N: int, K: int, x) -> None:
    """The codes [E, N, K / per] and scales of one quantized expert tensor as the kernels load them."""
    mult, cdt, per, name = _MOE_QUANT[fmt]
    if K % mult:
        raise ValueError(f"{what}: {name} expert rows of {K} inputs; a multiple of {mult} required (H and I both)")
    if Wq.dtype != cdt or tuple(Wq.shape) != (E, N, K // per):
        raise ValueError(f"{what}: {name} codes must be {cdt} [{E}, {N}, {K // per}], got {Wq.dtype} {tuple(Wq.shape)}")
    sshape, sdt = ((E, N), torch.float32) if fmt == "q8" else ((E, N, K // MX4_BLOCK), torch.uint8)
    if S.dtype != sdt or tuple(S.shape) != sshape:
        raise ValueError(f"{what}: {name} scales must be {sdt} {list(sshape)}, got {S.dtype} {tuple(S.shape)}")
    for nm, t in (("codes", Wq), ("scales", S)):
        if not t.is_cuda or t.device != x.device:
            raise ValueError(f"{what}: the {name} {nm} must be on the GPU with x, they are on {t.device}")
    if Wq.stride(-1) != 1 or Wq.stride(0) % 16 or Wq.stride(1) % 16 or Wq.data_ptr() % 16:
        raise ValueError(f"{what}: {name} codes {tuple(Wq.shape)} with strides {Wq.stride()} at offset "
                         f"{Wq.data_ptr() % 16} of a 16-byte line: unit inner stride, row and expert strides that are "
                         f"multiples of 16 bytes and a 16-byte aligned base required")
    if S.stride(-1) != 1 or (fmt == "q8" and S.data_ptr() % 4):
        raise ValueError(f"{what}: {name} scales {tuple(S.shape)} with strides {S.stride()}: unit inner stride required")


def _moe_act_out(what: str, out, rows: int, k: int, I: int, device):
    act = out if out is not None else torch.empty((rows, k, I), dtype=torch.float32, device=device)
    if (act.dtype != torch.float32 or tuple(act.shape) != (rows, k, I) or not act.is_contiguous() or not act.is_cuda
            or act.data_ptr() % 16):
        raise ValueError(f"{what}: out must be a contiguous, 16-byte aligned fp32 [{rows}, {k}, {I}] on the GPU, got "
                         f"{act.dtype} {tuple(act.shape)} on {act.device}")
    return act


def _moe_glu_quant(fmt: str, x, idx, Wq, S, rms_eps, gamma, out):
    what = "moe_glu_" + fmt
    if x.dim() != 2 or Wq.dim() != 3 or Wq.shape[1] % 2 or idx.dim() != 2:
        raise ValueError(f"{what}: x [rows, H], idx [rows, k] and codes [E, 2I, .] required, got {tuple(x.shape)}, "
                         f"{tuple(idx.shape)} and {tuple(Wq.shape)}")
    rows, H = x.shape
    _moe_gamma(what, gamma, rms_eps, H)
    if not x.is_cuda:
        ref = moe_glu_q8_ref if fmt == "q8" else moe_glu_mx4_ref
        return ref(x, idx, Wq, S, rms_eps, gamma)
    E, I, k = Wq.shape[0], Wq.shape[1] // 2, idx.shape[1]
    _moe_dims(what, rows, E, H, I, k)
    if I % _MOE_QUANT[fmt][0]:
        raise ValueError(f"{what}: I = {I}; a multiple of {_MOE_QUANT[fmt][0]} required (H and I both)")
    _moe_idx(what, idx, rows)
    _moe_refuse(what, x=x, gamma=gamma)
    _moe_quant_weights(what, fmt, Wq, S, E, 2 * I, H, x)
    act = _moe_act_out(what, out, rows, k, I, x.device)
    L = _lib.lib()
    if fmt == "q8":
        _lib.check(L.nos_moe_glu_q8(x.data_ptr(), x.stride(0), idx.data_ptr(), Wq.data_ptr(), Wq.stride(0), Wq.stride(1),
                                    S.data_ptr(), S.stride(0), _ptr(gamma), float(rms_eps), act.data_ptr(), rows, E, H, I,
                                    k, _stream()), "nos_moe_glu_q8")
    else:
        _lib.check(L.nos_moe_glu_mx4(x.data_ptr(), x.stride(0), idx.data_ptr(), Wq.data_ptr(), Wq.stride(0), Wq.stride(1),
                                     S.data_ptr(), S.stride(0), S.stride(1), _ptr(gamma), float(rms_eps), act.data_ptr(),
                                     rows, E, H, I, k, _stream()), "nos_moe_glu_mx4")
    return act


def _moe_down_quant(fmt: str, act, idx, w, Wq, S, res, out):
    what = "moe_down_" + fmt
    if (act.dim() != 3 or Wq.dim() != 3 or tuple(w.shape) != tuple(act.shape[:2])
            or tuple(idx.shape) != tuple(act.shape[:2])):
        raise ValueError(f"{what}: act [rows, k, I], idx and w [rows, k] and codes [E, H, .] required, got "
                         f"{tuple(act.shape)}, {tuple(idx.shape)}, {tuple(w.shape)} and {tuple(Wq.shape)}")
    rows, k, I = act.shape
    E, H = Wq.shape[:2]
    if res is not None and tuple(res.shape) != (rows, H):
        raise ValueError(f"{what}: res must be [{rows}, {H}], got {tuple(res.shape)}")
    if not act.is_cuda:
        ref = moe_down_q8_ref if fmt == "q8" else moe_down_mx4_ref
        y = ref(act, idx, w, Wq, S, res)
        return y if out is None else out.copy_(y)
    _moe_dims(what, rows, E, H, I, k)
    if H % _MOE_QUANT[fmt][0]:
        raise ValueError(f"{what}: H = {H}; a multiple of {_MOE_QUANT[fmt][0]} required (H and I both)")
    _moe_idx(what, idx, rows, k)
    if not act.is_contiguous() or not w.is_contiguous() or w.dtype != torch.float32 or not w.is_cuda:
        raise ValueError(f"{what}: act and w must be contiguous and w fp32 on the GPU, got w {w.dtype} on {w.device}")
    _moe_refuse(what, act=act)
    _moe_quant_weights(what, fmt, Wq, S, E, H, I, act)
    y = out if out is not None else torch.empty((rows, H), dtype=torch.float32, device=act.device)
    for name, t in (("res", res), ("out", y)):
        if t is not None and (t.dtype != torch.float32 or not t.is_cuda or t.stride(-1) != 1 or tuple(t.shape) != (rows, H)
                              or t.stride(0) < H):
            raise ValueError(f"{what}: {name} must be an fp32 [{rows}, {H}] on the GPU with unit inner stride, got "
                             f"{t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    L = _lib.lib()
    tail = (_ptr(res), res.stride(0) if res is not None else 0, y.data_ptr(), y.stride(0), rows, E, H, I, k, _stream())
    if fmt == "q8":
        _lib.check(L.nos_moe_down_q8(act.data_ptr(), idx.data_ptr(), w.data_ptr(), Wq.data_ptr(), Wq.stride(0),
                                     Wq.stride(1), S.data_ptr(), S.stride(0), *tail), "nos_moe_down_q8")
    else:
        _lib.check(L.nos_moe_down_mx4(act.data_ptr(), idx.data_ptr(), w.data_ptr(), Wq.data_ptr(), Wq.stride(0),
                                      Wq.stride(1), S.data_ptr(), S.stride(0), S.stride(1), *tail), "nos_moe_down_mx4")
    return y


def moe_glu_q8(x: torch.Tensor, idx: torch.Tensor, W13q: torch.Tensor, s13: torch.Tensor, rms_eps: float = 0.0,
               gamma: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`moe_glu` over int8 experts: W13q [E, 2I, H] i8 with one fp32 scale per row, s13 [E, 2I]
    (decode.hip ``nos_moe_glu_q8``; H % 16 == 0 and I % 16 == 0, codes with 16-byte rows).  One byte of
    HBM per weight of the chosen experts; fp32 FMAs on the int8 values, the row scale after the sum.  A
    slot outside [0, E) reads no weight or scale and is zeros.  CPU tensors: :func:`moe_glu_q8_ref`."""
    return _moe_glu_quant("q8", x, idx, W13q, s13, rms_eps, gamma, out)


def moe_down_q8(act: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, W2q: torch.Tensor, s2: torch.Tensor,
                res: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`moe_down` over int8 experts: W2q [E, H, I] i8, s2 [E, H] fp32 (decode.hip
    ``nos_moe_down_q8``); the slots summed in the order 0 .. k - 1 without atomics.  CPU tensors:
    :func:`moe_down_q8_ref`."""
    return _moe_down_quant("q8", act, idx, w, W2q, s2, res, out)


def moe_glu_mx4(x: torch.Tensor, idx: torch.Tensor, W13c: torch.Tensor, W13e: torch.Tensor, rms_eps: float = 0.0,
                gamma: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`moe_glu` over MXFP4 experts: codes W13c [E, 2I, H / 2] u8 and block scales W13e [E, 2I, H / 32]
    u8 (decode.hip ``nos_moe_glu_mx4``; H % 32 == 0 and I % 32 == 0).  4.25 bits of HBM per weight of the
    chosen experts, fp32 FMAs on the dequantized values.  Every scale byte must lie in [2, 252] (a
    registration checks it; this call does not read them).  CPU tensors: :func:`moe_glu_mx4_ref`."""
    return _moe_glu_quant("mx4", x, idx, W13c, W13e, rms_eps, gamma, out)


def moe_down_mx4(act: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, W2c: torch.Tensor, W2e: torch.Tensor,
                 res: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`moe_down` over MXFP4 experts: codes W2c [E, H, I / 2] u8, block scales W2e [E, H, I / 32] u8
    (decode.hip ``nos_moe_down_mx4``).  CPU tensors: :func:`moe_down_mx4_ref`."""
    return _moe_down_quant("mx4", act, idx, w, W2c, W2e, res, out)


def _moe_dense_quant(x, Wr, k: int, E: int, expert):
    """:func:`moe`'s dense path with ``expert(e)`` -> (W13 [2I, H], W2 [H, I]) fp32, made per expert and
    dropped after its product: one expert's fp32 weights alive at a time, never all of them."""
    x2 = x.reshape(-1, x.shape[-1])
    idx, w = moe_route_ref(x2, Wr, k)
    gates = torch.zeros((x2.shape[0], E), dtype=x2.dtype, device=x.device).scatter_(1, idx.long(), w)
    y = torch.zeros_like(x2)
    for e in range(E):
        W13, W2 = expert(e)
        I = W13.shape[0] // 2
        gu = x2 @ W13.T
        y = y + gates[:, e:e + 1] * ((F.silu(gu[:, :I]) * gu[:, I:]) @ W2.T)
        del W13, W2
    return y.view(x.shape)


def moe_q8(x: torch.Tensor, Wr: torch.Tensor, W13q: torch.Tensor, s13: torch.Tensor, W2q: torch.Tensor,
           s2: torch.Tensor, k: int) -> torch.Tensor:
    """``moe_q8`` (:func:`moe_q8_ref`) of fp32 x [..., H] on the device for steps of more rows than the
    kernels take (a prefill): :func:`moe`'s dense PyTorch path, one expert at a time dequantized into a
    transient fp32 buffer by the ``dequant_q8`` kernel (never all experts at once), no host read of a
    routing value.  CPU tensors: the reference."""
    if not x.is_cuda:
        return moe_q8_ref(x, Wr, W13q, s13, W2q, s2, k)
    return _moe_dense_quant(x, Wr, k, W13q.shape[0], lambda e: (dequant_q8(W13q[e], s13[e]), dequant_q8(W2q[e], s2[e])))


def moe_mx4(x: torch.Tensor, Wr: torch.Tensor, W13c: torch.Tensor, W13e: torch.Tensor, W2c: torch.Tensor,
            W2e: torch.Tensor, k: int) -> torch.Tensor:
    """``moe_mx4`` (:func:`moe_mx4_ref`) of fp32 x [..., H] for steps of more rows than the kernels take:
    as :func:`moe_q8`, with the ``dequant_mx4`` kernel.  CPU tensors: the reference."""
    if not x.is_cuda:
        return moe_mx4_ref(x, Wr, W13c, W13e, W2c, W2e, k)
    return _moe_dense_quant(x, Wr, k, W13c.shape[0],
                            lambda e: (dequant_mx4(W13c[e], W13e[e]), dequant_mx4(W2c[e], W2e[e])))


def set_attention_h3g_kvsplit(n: int) -> None:
    """Key splits of :func:`sdpa` and ``sdpa_cache(flash=True)`` (0 = auto: fill the CU slots)."""
    _lib.check(_lib.lib().nos_attn_h3g_set_kvsplit(int(n)), "nos_attn_h3g_set_kvsplit")


__all__ = ["glu", "kv_write", "rotary_at", "sdpa_cache", "cache_flash_rule", "sdpa_cache_flash_workspace_bytes",
           "pos_update", "argmax", "sample", "sample_row_ref",
           "sampling_ctl", "philox4x32", "gemv", "gemv_ok", "gemv_partials", "gemv_q8", "gemv_q8_ok", "gemv_q8_partials",
           "dequant_q8", "linear_q8", "linear_q8_ref", "gemv_mx4", "gemv_mx4_ok", "gemv_mx4_partials", "dequant_mx4",
           "linear_mx4", "linear_mx4_ref","lora", "lora_ref", "lora_shrink", "lora_shrink_ref", "lora_expand_ref", "linear_lora",
           "LORA_MAX_RANK", "moe", "moe_ref", "moe_route", "moe_glu", "moe_down", "moe_route_ref", "moe_glu_ref",
           "moe_down_ref", "MOE_MAX_EXPERTS", "MOE_MAX_TOP_K",
           "moe_q8", "moe_mx4", "moe_q8_ref", "moe_mx4_ref", "moe_glu_q8", "moe_down_q8", "moe_glu_mx4", "moe_down_mx4",
           "moe_glu_q8_ref", "moe_down_q8_ref", "moe_glu_mx4_ref", "moe_down_mx4_ref",
           "DecodePartials", "conv2d", "matmul", "sdpa", "linear_rms", "embedding", "rmsnorm", "softmax", "rotary", "conv2d_ref",
           "sdpa_ref", "rope_ref", "rmsnorm_ref", "linear_rms_ref", "set_attention_h3g_kvsplit", "EPI_BIAS_ROW",
           "sdpa_lse", "sdpa_bwd", "sdpa_lse_ref", "sdpa_bwd_ref", "sdpa_bwd_workspace_bytes"]
