"""Quantized experts on gfx950 (csrc/hip/decode.hip ``moe_glu_quant_kernel`` / ``moe_down_quant_kernel``
behind ``nos_moe_glu_q8``, ``nos_moe_down_q8``, ``nos_moe_glu_mx4``, ``nos_moe_down_mx4``): each kernel
against ``moe_*_ref`` on the dequantized experts in fp64 at the project's bar (``test_moe_gpu._close``: 4x
torch-fp32's own error, at least 2e-6 of max |y|; model logits: at least 1e-5), then the compiled
tenants and the GPU pod server against ``dequantized_llama(model, experts=...)`` in fp64.

No input sits on a tie: the kernel inputs come from ``test_moe_gpu._inputs`` (the routing gap asserted in
fp64), the model tests use ``test_moe``'s prompts through ``reference_run`` (both gaps asserted)."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402
from nos_amd.ops import _lib, _stream  # noqa: E402
from nos_amd.ops import tenant as T  # noqa: E402
from nos_amd.podserver.program import quantize_rows_mx4, quantize_rows_q8  # noqa: E402
from test_moe import (MAX_LEN, MIN_GAP, MIN_ROUTE_GAP, MODEL_SEED, NEW, PROMPT_LEN, prompt, reference_run)  # noqa: E402
from test_moe_gpu import (EPS, SENT, VARIANTS, _close, _compiled, _guarded, _guards_intact, _inputs, _logits_close,  # noqa: E402
                          _padded)

FORMATS = ("int8", "mxfp4")
# (rows, E, k, H, I), the smallest at which the kernels can still go wrong.  int8 (a lane: 16 k, a wave load:
# 1024 k): 4 busy lanes and one column group; lane tails in both kernels; one full wave load plus a 16-k tail
# with k = E (and two columns a wave in down); the tail on the down side with an odd k; a single row.
# MXFP4 (narrow form up to 1024 k: 16 k a lane; wide: 32 k a lane, 2048 k a wave load): one block; tails; past
# the narrow form's 1024 by one block; past a wide wave load by one block on the down side; a single row.
SHAPES = {"int8": [(1, 2, 1, 64, 16), (3, 5, 2, 208, 112), (8, 8, 8, 1040, 352), (8, 5, 5, 64, 1040), (1, 8, 2, 1024, 112)],
          "mxfp4": [(1, 2, 1, 32, 32), (3, 5, 2, 224, 96), (8, 8, 8, 1056, 352), (8, 5, 5, 64, 2080), (1, 8, 2, 2080, 96)]}
CASES = [(f, *s) for f in FORMATS for s in SHAPES[f]]
TINY = 2.0 ** -124


@pytest.fixture(autouse=True)
def _h3():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)


def _quantize(fmt, W):
    """(codes, scales) of the fp32 experts W [E, N, K] on the CPU, by the builder's rule on the flattened rows."""
    E, N, K = W.shape
    q, s = (quantize_rows_q8 if fmt == "int8" else quantize_rows_mx4)(W.reshape(E * N, K).numpy())
    return torch.from_numpy(q).view(E, N, -1), torch.from_numpy(s).view(E, N, *s.shape[1:])


def _dequantize(fmt, q, s):
    return T._dequant_experts_q8(q, s) if fmt == "int8" else T._dequant_experts_mx4(q, s)


def _quant_inputs(fmt, rows, E, k, H, I, **v):
    """``_inputs`` (the routing gap asserted) with the experts quantized: (x, Wr, (q13, s13), (q2, s2), gamma, res)
    on the CPU.  int8: -127 and 127 both occur (asserted).  MXFP4: the scale bytes 252 and 2 are planted in
    every expert (both occur, asserted) so that every value stays a NORMAL fp32 and every output O(1):
      * x[:, 0] = 2^-124 (1 .. 2); gate row 0 is the single element 1.5 x 2^125 at k = 0 (scale byte 252), so
        g_0 = 3 .. 6 times gamma_0 rsc; up row 0 is the single element 1.0 at k = 0, so u_0 = x_0' and
        act[:, :, 0] ~ 10 x 2^-124;
      * W2's row 0 starts with a block of the single element 0.5 x 2^125 at i = 0 (scale byte 252): its
        product with act[:, :, 0] is O(10);
      * the last block of gate row 1 and of W2's row 1 keeps its codes under the scale byte 2."""
    mx4 = fmt == "mxfp4"

    def make_x(_Wr, g):
        x = torch.randn(rows, H, generator=g)
        x[:, 0] = TINY * (1 + torch.rand(rows, generator=g))
        return x

    x, Wr, W13, W2, gm, res = _inputs(rows, E, k, H, I, make_x=make_x if mx4 else None, **v)
    (q13, s13), (q2, s2) = _quantize(fmt, W13), _quantize(fmt, W2)
    if not mx4:
        for q in (q13, q2):
            assert int(q.min()) == -127 and int(q.max()) == 127
        return x, Wr, (q13, s13), (q2, s2), gm, res
    q13[:, 0, :], q13[:, I, :] = 0, 0
    q13[:, 0, 0], q13[:, I, 0] = 3, 2      # the codes of 1.5 and of 1.0, element 0: the low nibble of byte 0
    s13[:, 0, :], s13[:, I, :] = 127, 127
    s13[:, 0, 0] = 252
    s13[:, 1, -1] = 2
    q2[:, 0, :16] = 0
    q2[:, 0, 0] = 1                        # the code of 0.5
    s2[:, 0, 0] = 252
    s2[:, 1, -1] = 2
    for s in (s13, s2):
        assert int(s.min()) == 2 and int(s.max()) == 252
    return x, Wr, (q13, s13), (q2, s2), gm, res


def _fns(fmt):
    return (T.moe_glu_q8, T.moe_down_q8) if fmt == "int8" else (T.moe_glu_mx4, T.moe_down_mx4)


def _pad_scales(fmt, s):
    return _padded(s, (0, 3) if fmt == "int8" else (0, 1, 3))[0]


def _run_block(fmt, x, Wr, w13, w2, gm, res, k, eps, idx_in=None):
    """The three launches on padded operands (a distinct leading dimension for each) with guarded outputs:
    (idx, w, act, y, y + res) and the sentinel checks.  ``idx_in``: route's indices replaced by these."""
    rows, H = x.shape
    I = w13[0].shape[1] // 2
    glu, down = _fns(fmt)
    xg, _ = _padded(x, (0, 8))
    wrg, _ = _padded(Wr, (0, 4))
    q13, _ = _padded(w13[0], (0, 2, 16))
    q2, _ = _padded(w2[0], (0, 1, 32))
    s13, s2 = _pad_scales(fmt, w13[1]), _pad_scales(fmt, w2[1])
    gg = None if gm is None else gm.cuda()
    (idx, ibuf), (w, wbuf), (act, abuf) = _guarded((rows, k), torch.int32), _guarded((rows, k), torch.float32), \
        _guarded((rows, k, I), torch.float32)
    T.moe_route(xg, wrg, k, eps, gg, out=(idx, w))
    if idx_in is not None:
        idx.copy_(idx_in)
    glu(xg, idx, q13, s13, eps, gg, out=act)
    ys = []
    for r in (None, res):
        rg = None if r is None else _padded(r, (0, 4))[0]
        y, ybuf = _padded(torch.zeros(rows, H), (0, 4))
        ybuf.fill_(SENT)
        down(act, idx, w, q2, s2, res=rg, out=y)
        assert bool((ybuf[:, H:] == SENT).all()), "moe_down wrote past its row"
        ys.append(y)
    torch.cuda.synchronize()
    assert _guards_intact(ibuf) and _guards_intact(wbuf) and _guards_intact(abuf), "a kernel wrote outside its output"
    return idx, w, act, ys[0], ys[1]


def _check_block(fmt, x, Wr, w13, w2, gm, res, k, eps, what):
    idx, w, act, y, yr = _run_block(fmt, x, Wr, w13, w2, gm, res, k, eps)
    d = torch.float64
    W13, W2 = _dequantize(fmt, *w13), _dequantize(fmt, *w2)   # fp32, the formats' definition
    idx64, _ = T.moe_route_ref(x, Wr, k, eps, gm, d)
    assert torch.equal(idx.cpu(), idx64), (what, idx.cpu().tolist(), idx64.tolist())
    _close(act, T.moe_glu_ref(x, idx64, W13, eps, gm, d), T.moe_glu_ref(x, idx64, W13, eps, gm), (what, "glu"))
    ac, wc = act.cpu(), w.cpu()   # the down kernel on the inputs it was given
    _close(y, T.moe_down_ref(ac, idx64, wc, W2, None, d), T.moe_down_ref(ac, idx64, wc, W2), (what, "down"))
    _close(yr, T.moe_down_ref(ac, idx64, wc, W2, res, d), T.moe_down_ref(ac, idx64, wc, W2, res), (what, "down + res"))
    xp64 = T._moe_x(x, eps, gm, d)
    _close(y, T.moe_ref(xp64, Wr.double(), W13.double(), W2.double(), k),
           T.moe_ref(T._moe_x(x, eps, gm, torch.float32), Wr, W13, W2, k), (what, "block"))
    return idx, w, act, y, yr


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("fmt, rows, E, k, H, I", CASES)
def test_quantized_kernels_match_fp64(fmt, rows, E, k, H, I):
    for v in VARIANTS:
        ins = _quant_inputs(fmt, rows, E, k, H, I, **v)
        _check_block(fmt, *ins, k, v.get("rms_eps", 0.0), (fmt, rows, E, k, H, I, tuple(v)))


@pytest.mark.parametrize("fmt", FORMATS)
def test_two_runs_are_bit_identical(fmt):
    ins = _quant_inputs(fmt, 8, 8, 2, 1024, 352, rms_eps=EPS, gamma=True)
    a = _run_block(fmt, *ins, 2, EPS)
    b = _run_block(fmt, *ins, 2, EPS)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_row_the_same_expert_and_every_row_another(fmt):
    rows, E, H, I = 8, 8, 224, 96

    def same(Wr, g):   # one direction plus a little noise: every row ranks the experts alike
        return 6 * torch.randn(1, H, generator=g) + 0.001 * torch.randn(rows, H, generator=g)

    def other(Wr, g):   # row m along the router's row m: expert m first
        return 3 * Wr / Wr.pow(2).sum(-1, keepdim=True) + 0.1 * torch.randn(rows, H, generator=g)

    for k in (1, 2):
        for make_x in (same, other):
            x, Wr, W13, W2, gm, res = _inputs(rows, E, k, H, I, make_x=make_x)
            idx = _check_block(fmt, x, Wr, _quantize(fmt, W13), _quantize(fmt, W2), gm, res, k, 0.0,
                               (fmt, make_x.__name__, k))[0].cpu()
            if make_x is same:
                assert bool((idx == idx[0]).all())
            else:
                assert idx[:, 0].tolist() == list(range(rows))


@pytest.mark.parametrize("fmt", FORMATS)
def test_unselected_experts_are_never_read(fmt):
    """Other in-range bytes in the codes and scales of every expert no row chose: every output bit-identical."""
    rows, E, k, H, I = 3, 8, 2, 224, 96
    x, Wr, w13, w2, gm, res = _quant_inputs(fmt, rows, E, k, H, I, rms_eps=EPS, gamma=True)
    chosen = set(T.moe_route_ref(x, Wr, k, EPS, gm, torch.float64)[0].flatten().tolist())
    idle = [e for e in range(E) if e not in chosen]
    assert idle
    g = torch.Generator().manual_seed(5)

    def scrambled(q, s):
        q2, s2 = q.clone(), s.clone()
        for e in idle:
            if fmt == "int8":
                q2[e] = torch.randint(-127, 128, q[e].shape, generator=g, dtype=torch.int8)
                s2[e] = torch.rand(s[e].shape, generator=g) + 0.5
            else:
                q2[e] = torch.randint(0, 256, q[e].shape, generator=g, dtype=torch.uint8)
                s2[e] = torch.randint(2, 253, s[e].shape, generator=g, dtype=torch.uint8)
            assert not torch.equal(q2[e], q[e]) and not torch.equal(s2[e], s[e])
        return q2, s2

    a = _run_block(fmt, x, Wr, w13, w2, gm, res, k, EPS)
    b = _run_block(fmt, x, Wr, scrambled(*w13), scrambled(*w2), gm, res, k, EPS)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bad", [-1, "E", 2 ** 30])
def test_an_index_outside_the_experts_contributes_zero(fmt, bad):
    rows, E, k, H, I = 3, 5, 3, 224, 96
    bad = E if bad == "E" else bad
    x, Wr, w13, w2, gm, res = _quant_inputs(fmt, rows, E, k, H, I)
    idx = T.moe_route_ref(x, Wr, k, dtype=torch.float64)[0].clone()
    idx[1, 1] = bad                     # one slot of one row
    _, w, act, y, yr = _run_block(fmt, x, Wr, w13, w2, gm, res, k, 0.0, idx_in=idx.cuda())   # the guards are checked
    assert bool((act[1, 1] == 0).all()) and bool((act[1, 0] != 0).any()) and bool((act[0, 1] != 0).any())
    W13, W2 = _dequantize(fmt, *w13), _dequantize(fmt, *w2)
    d = torch.float64
    _close(act, T.moe_glu_ref(x, idx, W13, dtype=d), T.moe_glu_ref(x, idx, W13), (fmt, bad, "glu"))
    # down: the reference without that slot -- its act replaced by NaN is never read either
    noise = act.clone()
    noise[1, 1] = float("nan")
    _, down = _fns(fmt)
    yn = down(noise, idx.cuda(), w, w2[0].cuda(), w2[1].cuda(), res=res.cuda())
    assert bool(torch.isfinite(yn).all()) and torch.equal(yn, yr.contiguous())
    keep = torch.ones(rows, k, dtype=torch.bool)
    keep[1, 1] = False
    ac, wc = act.cpu(), w.cpu() * keep   # the slot's weight zeroed, its index made valid: the sum without it
    valid = idx.clamp(0, E - 1)
    _close(yr, T.moe_down_ref(ac, valid, wc, W2, res, d), T.moe_down_ref(ac, valid, wc, W2, res), (fmt, bad, "down"))
    _close(yr, T.moe_down_ref(ac, idx, w.cpu(), W2, res, d), T.moe_down_ref(ac, idx, w.cpu(), W2, res), (fmt, bad, "down, idx"))


# ------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize("fmt", FORMATS)
def test_wrappers_refuse_what_the_kernels_do_not_take(fmt):
    m = 16 if fmt == "int8" else 32
    H, I = 4 * m, 2 * m
    x, Wr, w13, w2, _, _ = _quant_inputs(fmt, 3, 5, 2, H, I)
    x, Wr, q13, s13, q2, s2 = (t.cuda() for t in (x, Wr, *w13, *w2))
    glu, down = _fns(fmt)
    idx, w = T.moe_route(x, Wr, 2)
    act = glu(x, idx, q13, s13)
    y = down(act, idx, w, q2, s2)
    assert act.shape == (3, 2, I) and y.shape == (3, H)
    per = 1 if fmt == "int8" else 2

    def experts(E, N, K):   # well-formed codes and scales of another shape
        q = torch.zeros(E, N, K // per, dtype=q13.dtype, device="cuda")
        s = torch.ones(E, N, device="cuda") if fmt == "int8" else torch.full((E, N, K // 32), 127, dtype=torch.uint8, device="cuda")
        return q, s

    off = torch.zeros(q13.numel() + 16, dtype=q13.dtype, device="cuda")[8:8 + q13.numel()].view(q13.shape).copy_(q13)
    wide13 = torch.zeros(5, 2 * I, q13.shape[2] + 8, dtype=q13.dtype, device="cuda")[:, :, :q13.shape[2]]   # rows off 16 bytes
    big = (16384 + m) // m * m
    cases = [
        lambda: glu(x.bfloat16(), idx, q13, s13), lambda: glu(x, idx, q13.float(), s13),                # dtypes
        lambda: glu(x, idx, q13, s13.double() if fmt == "int8" else s13.float()),
        lambda: glu(x, idx.long(), q13, s13),
        lambda: glu(x, idx, q13.cpu(), s13), lambda: glu(x, idx, q13, s13.cpu()),                        # devices
        lambda: glu(x, idx, off, s13),                                                                   # a misaligned base
        lambda: glu(x, idx, wide13, s13),                                                                # a row stride off 16 bytes
        lambda: glu(x, idx, q13.transpose(1, 2).contiguous().transpose(1, 2), s13),                      # inner stride
        lambda: glu(x, idx, q13, s13.transpose(0, 1).contiguous().transpose(0, 1)) if fmt == "int8"
        else glu(x, idx, q13, s13.transpose(1, 2).contiguous().transpose(1, 2)),                         # the scales' inner stride
        lambda: glu(x, idx, q13, s13[:, :-1]),                                                           # the scales' shape
        lambda: glu(x[:, :H - m // 2].contiguous(), idx, *experts(5, 2 * I, H - m // 2)),                 # H off the rule
        lambda: glu(x, idx, *experts(5, 2 * (I - m // 2), H)),                                           # I off the rule
        lambda: glu(torch.randn(9, H, device="cuda"), torch.zeros(9, 2, dtype=torch.int32, device="cuda"), q13, s13),   # rows
        lambda: glu(torch.randn(1, big, device="cuda"), idx[:1], *experts(2, 2 * m, big)),               # H x 4 > 64 KiB
        lambda: down(torch.randn(1, 8, 2048 + m, device="cuda"), torch.zeros(1, 8, dtype=torch.int32, device="cuda"),
                     torch.ones(1, 8, device="cuda"), *experts(8, m, 2048 + m)),                         # k x I x 4 > 64 KiB
        lambda: glu(x, idx, q13, s13, gamma=torch.ones(H, device="cuda")),                               # gamma without rms_eps
        lambda: down(act, idx, w, q2.float(), s2), lambda: down(act, idx, w.double(), q2, s2),
        lambda: down(act, idx, w, q2, s2[:, :-1]), lambda: down(act, idx, w[:, :1], q2, s2),
        lambda: down(act, idx, w, q2, s2, res=torch.zeros(3, H - 4, device="cuda")),
        lambda: down(act.transpose(0, 1), idx, w, q2, s2),
        lambda: down(act, idx, w, q2, s2, out=torch.zeros(3, H, device="cuda", dtype=torch.bfloat16)),
        lambda: down(act, idx, w, *experts(5, H - m // 2, I)),                                           # H off the rule
    ]
    for n, call in enumerate(cases):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {n} was taken")
    # the entry points check for themselves (hipErrorInvalidValue = 1, nothing launched)
    L = _lib.lib()
    out = torch.full((3, H), SENT, device="cuda")
    s = _stream()
    ld13, ld2 = q13.stride(1), q2.stride(1)
    if fmt == "int8":
        assert L.nos_moe_glu_q8(x.data_ptr(), H, idx.data_ptr(), q13.data_ptr() + 4, q13.stride(0), ld13, s13.data_ptr(),
                                2 * I, None, 0.0, act.data_ptr(), 3, 5, H, I, 2, s) == 1
        assert L.nos_moe_glu_q8(x.data_ptr(), H, idx.data_ptr(), q13.data_ptr(), q13.stride(0) - 16, ld13, s13.data_ptr(),
                                2 * I, None, 0.0, act.data_ptr(), 3, 5, H, I, 2, s) == 1
        assert L.nos_moe_down_q8(act.data_ptr(), idx.data_ptr(), w.data_ptr(), q2.data_ptr(), q2.stride(0), ld2 + 8,
                                 s2.data_ptr(), H, None, 0, out.data_ptr(), H, 3, 5, H, I, 2, s) == 1
        assert L.nos_moe_down_q8(act.data_ptr(), idx.data_ptr(), w.data_ptr(), q2.data_ptr(), q2.stride(0), ld2,
                                 s2.data_ptr(), H - 1, None, 0, out.data_ptr(), H, 3, 5, H, I, 2, s) == 1
        assert L.nos_moe_down_q8(act.data_ptr(), idx.data_ptr(), w.data_ptr(), q2.data_ptr(), q2.stride(0), ld2,
                                 s2.data_ptr(), H, None, 0, out.data_ptr(), H, 9, 5, H, I, 2, s) == 1
    else:
        assert L.nos_moe_glu_mx4(x.data_ptr(), H, idx.data_ptr(), q13.data_ptr() + 4, q13.stride(0), ld13, s13.data_ptr(),
                                 s13.stride(0), s13.stride(1), None, 0.0, act.data_ptr(), 3, 5, H, I, 2, s) == 1
        assert L.nos_moe_glu_mx4(x.data_ptr(), H, idx.data_ptr(), q13.data_ptr(), q13.stride(0), ld13, s13.data_ptr(),
                                 s13.stride(0), H // 32 - 1, None, 0.0, act.data_ptr(), 3, 5, H, I, 2, s) == 1
        assert L.nos_moe_down_mx4(act.data_ptr(), idx.data_ptr(), w.data_ptr(), q2.data_ptr(), q2.stride(0), ld2 + 8,
                                  s2.data_ptr(), s2.stride(0), s2.stride(1), None, 0, out.data_ptr(), H, 3, 5, H, I, 2, s) == 1
        assert L.nos_moe_down_mx4(act.data_ptr(), idx.data_ptr(), w.data_ptr(), q2.data_ptr(), q2.stride(0), ld2,
                                  s2.data_ptr(), s2.stride(0) - 1, s2.stride(1), None, 0, out.data_ptr(), H, 3, 5, H, I, 2, s) == 1
        assert L.nos_moe_down_mx4(act.data_ptr(), idx.data_ptr(), w.data_ptr(), q2.data_ptr(), q2.stride(0), ld2,
                                  s2.data_ptr(), s2.stride(0), s2.stride(1), None, 0, out.data_ptr(), H, 3, 5, H, I, 9, s) == 1
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ------------------------------------------------------------------ 3. whole tenants
@pytest.fixture(scope="module")
def model():
    from nos_amd.models.llama_program import mixtral_config, mixtral_model

    return mixtral_model(mixtral_config(), MODEL_SEED)


@pytest.fixture(scope="module")
def references(model):
    """Per format: the dequantized-experts model and its fp64 greedy ids of ``prompt(2)`` (both gaps asserted)."""
    from nos_amd.models.llama_program import dequantized_llama

    out = {}
    for fmt in FORMATS:
        dm = dequantized_llama(model, experts=fmt)
        out[fmt] = (dm, reference_run(dm, prompt(2)))
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_step_and_prefill_logits_match_the_dequantized_model_in_fp64(fmt, model, references):
    """A prefill of 8 rows and three decode steps (the kernels), then a prefill of 16 rows (the dense path, one
    expert dequantized at a time, in every layer but the last)."""
    dm, ref = references[fmt]
    (pre, step), state = _compiled(model, experts=fmt)
    seq = torch.from_numpy(prompt()).long().cuda()
    with torch.no_grad():
        logits, nxt = pre(seq.int())
        _logits_close(logits, dm, seq, (fmt, "prefill 8"))
        for s in range(3):
            assert int(nxt) == int(ref[0, s])
            seq = torch.cat([seq, nxt.long().view(1, 1)], 1)
            logits, nxt = step(nxt.view(1, 1).int())
            _logits_close(logits, dm, seq, (fmt, f"step {s}"))
    assert state["pos"].tolist() == [PROMPT_LEN + 3]
    (pre16, _), state = _compiled(model, prompt_len=16, experts=fmt)
    L = model.config.num_hidden_layers
    op = "moe_q8" if fmt == "int8" else "moe_mx4"
    assert [s.kind for s in pre16.steps].count(op) == L - 1 and pre16.stats["moe_launches"] == 3
    seq = torch.from_numpy(np.concatenate([prompt(), ref[:1, :8]], 1)).long().cuda()
    with torch.no_grad():
        logits, nxt = pre16(seq.int())
    _logits_close(logits, dm, seq, (fmt, "prefill 16"))
    assert int(nxt) == int(ref[0, 8]) and state["pos"].tolist() == [16]


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_step_costs_the_fp32_expert_steps_launches(fmt, model):
    L = model.config.num_hidden_layers
    (_, fstep), _ = _compiled(model)
    (pre, step), _ = _compiled(model, experts=fmt)
    sfx = "_q8" if fmt == "int8" else "_mx4"
    for c in (pre, step):   # 8 rows and 1: both on the kernels
        st = c.stats
        assert st["moe_blocks"] == st["moe_rms_prologue"] == st["moe_residual_fused"] == L and st["moe_launches"] == 3 * L
        kinds = [s.kind for s in c.steps]
        assert kinds.count("moe_route") == kinds.count("moe_glu" + sfx) == kinds.count("moe_down" + sfx) == L
        assert not any(k in kinds for k in ("moe", "moe" + sfx, "moe_glu", "moe_down", "add", "rmsnorm"))
    assert step.stats["kernels"] == fstep.stats["kernels"]
    for k in ("rmsnorm_folded", "decode_combines_into_gemv", "kv_writes_into_attention", "pos_add_into_argmax",
              "rotary_at_fused"):
        assert step.stats.get(k) == fstep.stats.get(k), k
    # the steps read the stored params themselves: no fp32 copy of an expert tensor
    for s in step.steps:
        if s.kind.startswith(("moe_glu", "moe_down")):
            assert all(i in step.consts and step.consts[i].dtype != torch.float32 or i.endswith(".scale")
                       for i in s.inputs[2:4])
    assert not any(t.dtype == torch.float32 and t.dim() == 3 for t in step.consts.values())


def _reference_run_kvq8(m, ids, new=NEW):
    """``reference_run`` with int8 K / V caches: greedy fp64 ids of ``m`` run with ``kv_q8_roundtrip_cache()`` (a
    full recompute per token), the routing gap and the top-2 logit gap asserted on this reference alone."""
    from nos_amd.models.llama_program import kv_q8_roundtrip_cache

    m64 = copy.deepcopy(m).double()
    k = m64.config.num_experts_per_tok
    route_gap = [float("inf")]

    def hook(_mod, _inp, out):
        p = torch.softmax(out[0].double(), -1).sort(-1, descending=True).values
        route_gap[0] = min(route_gap[0], float((p[:, k - 1] - p[:, k]).min()))

    hooks = [layer.mlp.gate.register_forward_hook(hook) for layer in m64.model.layers]
    seq = torch.from_numpy(ids.astype(np.int64))
    gap = float("inf")
    with torch.no_grad():
        for _ in range(new):
            logits = m64(seq, past_key_values=kv_q8_roundtrip_cache()).logits[:, -1]
            top = logits.topk(2, dim=-1)
            gap = min(gap, float(((top.values[:, 0] - top.values[:, 1]) / logits.abs().amax(-1)).min()))
            seq = torch.cat([seq, top.indices[:, :1]], 1)
    for h in hooks:
        h.remove()
    assert route_gap[0] >= MIN_ROUTE_GAP, f"routing gap {route_gap[0]}: pick another seed"
    assert gap >= MIN_GAP, f"top-2 logit gap {gap}: pick another seed"
    return seq[:, ids.shape[1]:].numpy().astype(np.int32)


def test_gpu_server_generates_the_dequantized_models_tokens(model, references, tmp_path):
    """HIP graphs and the server loop for both formats; then int8 experts beside batch 2, int8 caches and
    speculation: the token count contract of its fp32-expert twin, the reference's tokens."""
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    srv = PodServer(tmp_path / "g.sock", device="cuda", lanes=2, memory_gb=40).start()

    def client(name, **kw):
        progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, **kw)
        c = PodClient(srv.path, connect_timeout_s=60)
        c.register(name, progs[0], w, memory_limit_gb=4, variants=progs[1:])
        return c

    try:
        for fmt in FORMATS:
            _, ref = references[fmt]
            c = client("moe-" + fmt, experts=fmt)
            for loop in (True, False):
                ids, tm = c.generate(prompt(), NEW, server_loop=loop)
                assert np.array_equal(ids, ref[:1]), (fmt, loop, ids, ref[:1])
                assert tm["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
                c.reset()
            c.close()
            c = client("moe-b2-" + fmt, experts=fmt, batch=2)
            got, _ = c.generate(prompt(2), NEW, server_loop=True)
            assert np.array_equal(got, ref), (fmt, got, ref)
            c.close()
        combo = dict(batch=2, kv="int8", speculate=4)
        want = _reference_run_kvq8(references["int8"][0], prompt(2))
        c = client("moe-eq8-combo", experts="int8", **combo)
        spec, t = c.generate(prompt(2), NEW, speculate=True)
        c.close()
        c = client("moe-fp32-combo", **combo)
        twin, tt = c.generate(prompt(2), NEW, speculate=True)
        c.close()
        assert spec.shape == twin.shape == (2, NEW) and t["steps_run"] <= NEW - 1 and tt["steps_run"] <= NEW - 1
        assert t["n_acc"].shape[1] == tt["n_acc"].shape[1] == 2
        assert t["state"] == tt["state"] == {"pos": [PROMPT_LEN + NEW - 1] * 2}
        assert np.array_equal(spec, want), (spec, want)
    finally:
        srv.stop()
