"""The fp16x3 ("h3") fp32 attention (csrc/hip/attention_f32x.hip,
csrc/hip/split_f16.h) against fp64 references: every fp32 operand as two
fp16 pieces on a power-of-two scale and three fp16 MFMAs per product, next to
the exact-f32 MFMA kernel and the bf16x6 kernel on the same inputs.  Its
error may not exceed the exact kernel's by more than 50 % (max and mean),
including inputs whose keys / values / queries sit far from 1 in magnitude
(the per-head scales come from the weights, the per-query scale from the
row)."""
from __future__ import annotations

import pytest
import torch

from nos_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _problem(B, S, H, K=384, wscale=0.05, xscale=2.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(B, S, K, generator=g) * xscale + 0.5).to(DEV)
    w = (torch.randn(3 * H * 64, K, generator=g) * wscale).to(DEV)
    b = (torch.randn(3 * H * 64, generator=g) * wscale * 4).to(DEV)
    gam = (1 + 0.2 * torch.randn(K, generator=g)).to(DEV)
    bet = (0.2 * torch.randn(K, generator=g)).to(DEV)
    return x, w, b, gam, bet


def _ref(x, w, b, gam, bet, H, eps=1e-12):
    B, S, K = x.shape
    xd = torch.nn.functional.layer_norm(x.cpu().double(), (K,), gam.cpu().double(), bet.cpu().double(), eps)
    qkv = xd @ w.cpu().double().t() + b.cpu().double()
    q, k, v = qkv.view(B, S, 3, H, 64).unbind(2)
    p = torch.softmax((q.transpose(1, 2) @ k.transpose(1, 2).transpose(-1, -2)) / 8.0, dim=-1)
    return (p @ v.transpose(1, 2)).transpose(1, 2).reshape(B, S, H * 64)


def _run(x, w, b, gam, bet, H, math_, variant):
    wg, c1, c2 = ops.fold_layernorm(w, b, gam, bet)
    ops.set_f32_math(math_)
    ops.set_attention_f32_variant(variant)
    try:
        if ops.ln_qkv_fusable(x):
            y = ops.ln_qkv_attention(x, wg, c1, c2, H)
        else:
            y = ops.attention_qkv(ops.linear_ln(x, wg, c1, c2), H)
        torch.cuda.synchronize()
    finally:
        ops.set_f32_math("exact")
        ops.set_attention_f32_variant("auto")
    return y


@pytest.mark.parametrize("wscale,xscale", [(0.05, 2.0), (2e-4, 1.0), (3.0, 1e3), (0.05, 1e-3)])
def test_h3_attention_is_as_accurate_as_exact_f32(wscale, xscale):
    """LN -> QKV -> attention at YOLOS-small's shape, fp64 reference: the h3
    attention's max and mean error within 1.5x of the x6 attention's on the
    same projection, and the all-h3 path's within 1.5x of the exact-f32
    path's, with
    weights from 2e-4 to 3 (keys and values from ~1e-2 to ~1e3; logits up to
    saturation) and inputs from 1e-3 to 1e3."""
    B, S, H = 1, 3401, 6
    x, w, b, gam, bet = _problem(B, S, H, wscale=wscale, xscale=xscale, seed=3)
    ref = _ref(x, w, b, gam, bet, H)
    errs = {}
    for name, math_, variant in (("exact", "exact", "w4k32o4"), ("x6", "x6", "x6n"), ("h3", "x6", "h3n"),
                                 ("h3gemm", "h3", "h3n")):
        e = (_run(x, w, b, gam, bet, H, math_, variant).cpu().double() - ref).abs()
        errs[name] = (e.max().item(), e.mean().item())
    print("attention error vs fp64 (max, mean):", errs)
    scale = ref.abs().max().item()
    # the h3 attention adds nothing to the x6 path's error (same x6 QKV GEMM) ...
    assert errs["h3"][0] <= 1.5 * errs["x6"][0] + 1e-7 * scale, errs
    assert errs["h3"][1] <= 1.5 * errs["x6"][1] + 1e-9 * scale, errs
    # ... and the all-h3 path (LayerNorm in the split pre-pass, two-pass
    # variance) is within the exact-f32 path's error even where the folded-LN
    # GEMMs lose digits to a large row mean (xscale 1e-3: mean 0.5, std 1e-3)
    assert errs["h3gemm"][0] <= 1.5 * errs["exact"][0] + 1e-7 * scale, errs
    assert errs["h3gemm"][1] <= 1.5 * errs["exact"][1] + 1e-9 * scale, errs


@pytest.mark.parametrize("variant", ["h3", "h3n", "h3k2", "h3k3", "h3k4"])
@pytest.mark.parametrize("B,S,H", [(1, 3401, 6), (2, 77, 3), (1, 1, 1), (3, 33, 2), (1, 129, 1)])
def test_h3_key_splits_and_tail_tiles(B, S, H, variant):
    """Every key-split count and tail-tile shape (S = 1, 33, 77, 129; batch
    padding between sequences) within fp32 accuracy of fp64."""
    x, w, b, gam, bet = _problem(B, S, H, seed=B * S + H)
    ref = _ref(x, w, b, gam, bet, H)
    y = _run(x, w, b, gam, bet, H, "x6", variant)
    err = (y.cpu().double() - ref).abs().max().item()
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("variant", ["h3k2", "h3k4"])
@pytest.mark.parametrize("B,S,H", [(2, 129, 1), (1, 33, 2)])
def test_h3_plane_output_under_forced_key_splits(B, S, H, variant):
    """The merge kernel's plane output (the proj GEMM's A planes instead of
    fp32 O) under a forced key split, at the tolerance of
    test_h3_key_splits_and_tail_tiles.  (2, 129, 1): a tail tile, five key
    tiles (four non-empty splits) and a batch stride of the K / V planes (160
    rows) that differs from S."""
    x, w, b, gam, bet = _problem(B, S, H, K=32, seed=B * S + H)
    ref = _ref(x, w, b, gam, bet, H)
    wg, c1, c2 = ops.fold_layernorm(w, b, gam, bet)
    ops.set_f32_math("x6")
    ops.set_attention_f32_variant(variant)
    try:
        p = ops.ln_qkv_attention(x, wg, c1, c2, H, planes_out=True)
        torch.cuda.synchronize()
    finally:
        ops.set_f32_math("exact")
        ops.set_attention_f32_variant("auto")
    assert p.shape == (B, S, H * 64) and p.rinv is None
    y = ((p.planes[0].cpu().double() + p.planes[1].cpu().double()) * p.rconst).view(B, S, H * 64)
    err = (y - ref).abs().max().item()
    print("plane output error vs fp64:", err)
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), err


def test_h3_planes_padding_rows_never_reach_the_output():
    """fp16 NaN in the planes' padding rows past S of each batch never
    reaches the output (the tail tile re-reads the last key)."""
    B, S, H, K = 2, 77, 3, 384
    x, w, b, gam, bet = _problem(B, S, H, seed=7)
    wg, c1, c2 = ops.fold_layernorm(w, b, gam, bet)
    ops.set_f32_math("x6")
    ops.set_attention_f32_variant("h3n")
    try:
        qkv, ws, sc = ops.linear_ln_qkv_h3(x, wg, c1, c2, H)
        ref = ops.attention_presplit_h3(qkv, ws, sc, H).clone()
        skvp = (S + 31) // 32 * 32
        row = 4 * H * 64  # fp16 elements per token row of the four planes
        planes = ws[:B * skvp * row].view(B, skvp, row)
        planes[:, S:, :] = 0x7E00  # fp16 NaN
        got = ops.attention_presplit_h3(qkv, ws, sc, H)
        torch.cuda.synchronize()
    finally:
        ops.set_f32_math("exact")
        ops.set_attention_f32_variant("auto")
    assert torch.isfinite(got).all() and torch.equal(got, ref)


def test_h3_yolos_tenant_matches_the_x6_tenant():
    """A YOLOS-small fp32 program compiled under the h3 attention: outputs
    within fp32 accuracy of the x6 attention's on the same weights."""
    from nos_amd.models.yolos_program import demo_tenant
    from nos_amd.podserver import program as PG

    prog, w = demo_tenant("fp32", 11, small=True)
    P = PG.parse(prog, w, gpu=True)
    x = torch.randn(*P.inputs[0].shape, generator=torch.Generator().manual_seed(2))
    outs = {}
    ops.set_f32_math("x6")
    try:
        for v in ("x6n", "h3n"):
            ops.set_attention_f32_variant(v)
            with torch.no_grad():
                outs[v] = [o.float().cpu() for o in P.compile("cuda")(P.input_tensor("cuda", x.numpy()))]
            torch.cuda.synchronize()
    finally:
        ops.set_f32_math("exact")
        ops.set_attention_f32_variant("auto")
    for a, c in zip(outs["x6n"], outs["h3n"]):
        assert (a - c).abs().max().item() <= 1e-4 * max(1.0, a.abs().max().item())
