"""The eager, unfused op semantics in PyTorch: the numerics reference of
:meth:`Program.reference` and the load-time constant folding."""
from __future__ import annotations

import os

from .ir import ProgramError, torch_dtype


def _eager(op: str, args: list, attrs: dict, ref: bool = False):
    """One unfused op in PyTorch (constant folding, and :meth:`Program.reference`)."""
    import torch
    import torch.nn.functional as F

    from ... import ops

    if op == "linear":
        y = F.linear(args[0], args[1], args[2] if len(args) > 2 else None)
        act = attrs.get("act")
        return F.gelu(y) if act == "gelu" else (F.relu(y) if act == "relu" else y)
    if op == "linear_q8":
        from ...ops import tenant as T

        return T.linear_q8(args[0], args[1], args[2], args[3] if len(args) > 3 else None, act=attrs.get("act"))
    if op == "linear_mx4":
        from ...ops import tenant as T

        return T.linear_mx4(args[0], args[1], args[2], args[3] if len(args) > 3 else None, act=attrs.get("act"))
    if op == "layernorm":
        x = args[0]
        return F.layer_norm(x, (x.shape[-1],), args[1], args[2], attrs.get("eps", 1e-5))
    if op == "attention":
        # fp32 under h3 math: the h3 flash kernel with per-row scales (a bare
        # attention has no LN-folded weights to bound K / V; the x6 kernel it
        # replaces spends six MFMAs per product instead of three)
        h3 = (args[0].is_cuda and args[0].dtype == torch.float32 and ops.f32_math() == "h3" and not ref
              and os.environ.get("NOS_AMD_BARE_ATTN_X6") != "1")   # (=1: the x6 kernel, for A/B)
        if (attrs.get("causal") or args[0].shape[-1] // (3 * attrs["heads"]) != 64 or not args[0].is_cuda
                or h3):
            from ...ops import tenant as T

            q, k, v = _qkv_views(args[0], attrs["heads"])
            if "q_start" in attrs:
                q = q[:, attrs["q_start"]:attrs["q_end"]]
            return T.sdpa(q, k, v, causal=attrs.get("causal", False), scale=attrs.get("scale")).flatten(2)
        y = ops.attention_qkv(args[0].contiguous(), attrs["heads"], scale=attrs.get("scale"))
        return y[:, attrs["q_start"]:attrs["q_end"]] if "q_start" in attrs else y
    if op == "add":
        return args[0] + args[1]
    if op == "mul":
        return args[0] * args[1]
    if op == "gelu":
        return F.gelu(args[0])
    if op == "relu":
        return F.relu(args[0])
    if op == "sigmoid":
        return torch.sigmoid(args[0])
    if op == "silu":
        return F.silu(args[0])
    if op == "cat":
        return torch.cat(args, dim=attrs["dim"])
    if op == "slice":
        d = attrs["dim"]
        return args[0].narrow(d, attrs["start"], attrs["end"] - attrs["start"])
    if op == "reshape":
        return args[0].reshape(attrs["shape"])
    if op == "permute":
        return args[0].permute(attrs["dims"])
    if op == "expand":
        return args[0].expand(attrs["shape"])
    if op == "cast":
        return args[0].to(torch_dtype(attrs["dtype"]))
    if op == "interpolate":
        mode = attrs.get("mode", "bicubic")
        return F.interpolate(args[0], size=tuple(attrs["size"]), mode=mode,
                             align_corners=None if mode == "nearest" else False)
    if op == "sub":
        return args[0] - args[1]
    if op == "div":
        return args[0] / args[1]
    if op == "tanh":
        return torch.tanh(args[0])
    if op == "exp":
        return torch.exp(args[0])
    if op == "neg":
        return -args[0]
    if op == "rsqrt":
        return torch.rsqrt(args[0])
    if op == "conv2d":
        return F.conv2d(args[0], args[1], args[2] if len(args) > 2 else None, _pair2(attrs, "stride", 1),
                        _pair2(attrs, "padding", 0), _pair2(attrs, "dilation", 1), attrs.get("groups", 1))
    if op == "batchnorm":
        return F.batch_norm(args[0], args[3], args[4], args[1], args[2], False, 0.0, attrs.get("eps", 1e-5))
    if op == "max_pool2d":
        k = _pair2(attrs, "kernel", 1)
        return F.max_pool2d(args[0], k, attrs.get("stride") and _pair2(attrs, "stride", 1) or k,
                            _pair2(attrs, "padding", 0))
    if op == "avg_pool2d":
        k = _pair2(attrs, "kernel", 1)
        return F.avg_pool2d(args[0], k, attrs.get("stride") and _pair2(attrs, "stride", 1) or k,
                            _pair2(attrs, "padding", 0))
    if op == "mean":
        return args[0].mean(dim=attrs["dims"], keepdim=attrs.get("keepdim", False))
    if op == "sum":
        return args[0].sum(dim=attrs["dims"], keepdim=attrs.get("keepdim", False))
    if op == "matmul":
        return args[0] @ args[1]
    if op == "softmax":
        return torch.softmax(args[0].float(), dim=-1).to(args[0].dtype)
    if op == "embedding":
        return F.embedding(args[0].long(), args[1])
    from ...ops import tenant as T

    if op == "rmsnorm":
        return T.rmsnorm_ref(args[0], args[1], attrs.get("eps", 1e-5))
    if op == "rotary":
        return T.rope_ref(args[0], args[1], args[2])
    if op == "sdpa":
        return T.sdpa_ref(args[0], args[1], args[2], attrs.get("causal", False), attrs.get("scale"))
    if op == "kv_write":
        return kv_write_ref(args[0], args[1], args[2], args[3] if len(args) > 3 else None,
                            window=attrs.get("window"), limit=attrs.get("limit"))
    if op == "sdpa_cache":
        return sdpa_cache_ref(args[0], args[1], args[2], args[3], attrs.get("scale"), *args[4:6],
                              window=attrs.get("window"), limit=attrs.get("limit"))
    if op == "rotary_at":
        return rotary_at_ref(args[0], args[1], args[2], args[3])
    if op == "pos_add" and len(args) == 2:   # a stopping tenant's: finished rows keep their counter
        T.stop_step(None, args[0], args[1], None, n=int(attrs["n"]), mode=2)
        return args[0]
    if op == "pos_add":
        return args[0].add_(int(attrs["n"]))
    if op == "seen_mark":
        return T.seen_mark(args[0], args[1], reset=bool(attrs.get("reset", False)))
    if op == "penalize":
        return T.penalize(args[0], args[1], args[2])
    if op == "stop_ids":
        return T.stop_ids(args[0], args[1], args[2])
    if op == "done_mark":
        return T.done_mark(args[0], args[1], args[2])
    if op == "hist_write":
        return T.hist_write(args[0], args[1], args[2], args[3] if len(args) > 3 else None,
                            args[4] if len(args) > 4 else None, back=int(attrs.get("back", 0)), lead=attrs.get("lead"))
    if op == "spec_accept":
        return T.spec_accept(args[0], args[1], args[2], args[3], int(attrs["limit"]))
    if op == "pos_advance":
        return T.pos_advance(args[0], args[1])
    if op == "spec_draft":
        return T.spec_draft(args[0], args[1], int(attrs["k"]))
    if op == "lora":
        return T.lora_ref(args[0], args[1], args[2], args[3])
    if op in ("moe_q8", "moe_mx4"):   # moe over the experts dequantized in fp32, in x's arithmetic
        return (T.moe_q8_ref if op == "moe_q8" else T.moe_mx4_ref)(*args[:6], int(attrs["top_k"]))
    if op == "moe":   # in x's arithmetic: fp32 for a program, fp64 when a test passes fp64 tensors
        return T.moe_ref(args[0], args[1], args[2], args[3], int(attrs["top_k"]))
    if op == "pos_set":
        return args[0].fill_(int(attrs["value"]))
    if op == "argmax":
        return args[0].float().argmax(dim=-1).to(torch.int32)
    if op == "sample":
        return T.sample(args[0], args[1], args[2].reshape(-1))
    raise ProgramError(f"op {op!r}")


def quantize_kv_rows(x):
    """The rows x [..., D] as an i8 cache stores them: ``builder.quantize_rows_q8``'s rule on each
    row, in fp32 whatever x's dtype -- (q int8 [..., D], scale fp32 [...])."""
    import torch

    xf = x.to(torch.float32)
    amax = xf.abs().amax(dim=-1)
    scale = torch.where(amax > 0, amax / 127, torch.ones_like(amax))
    q = torch.clamp(torch.round(xf / scale[..., None]), -127, 127).to(torch.int8)
    return q, scale


def dequantize_kv_rows(q, scale):
    """What an i8 cache holds: ``float(q) * scale`` in fp32, one rounding."""
    import torch

    return q.to(torch.float32) * scale.to(torch.float32)[..., None]


def _ring_args(what: str, window, limit, C: int, S: int) -> bool:
    """``window`` / ``limit`` of a ring cache of C slots at a step of S rows (both or neither; the
    validator's rule): whether the cache is a ring."""
    if (window is None) != (limit is None):
        raise ValueError(f"{what}: window and limit are given together (a ring cache), or neither")
    if window is None:
        return False
    if window < 1 or limit < 1 or C > limit or C < min(limit, window + S - 1):
        raise ValueError(f"{what}: a ring cache of {C} slots does not fit window {window}, limit {limit} and "
                         f"{S} rows a step (min(limit, window + S - 1) <= slots <= limit)")
    return True


def kv_write_ref(cache, x, pos, scales=None, window=None, limit=None):
    """cache[b, pos[b] + i] = x[b, i] for the rows that fit (in place).  An int8 cache with its
    ``scales`` [B, L, Hkv] (fp32): the rows quantized (:func:`quantize_kv_rows`) into both.

    ``window`` and ``limit``: the cache is a ring of C = L slots -- the row of position p goes to slot
    p % C, rows at p < 0 or p >= limit are dropped."""
    import torch

    q8 = cache.dtype == torch.int8
    if q8 != (scales is not None):
        raise ValueError("kv_write: an int8 cache, and only an int8 cache, takes scales")
    L, S = cache.shape[1], x.shape[1]
    if _ring_args("kv_write", window, limit, L, S):
        for b in range(cache.shape[0]):
            for i in range(S):
                p = int(pos[b]) + i
                if 0 <= p < limit:
                    if q8:
                        cache[b, p % L], scales[b, p % L] = quantize_kv_rows(x[b, i])
                    else:
                        cache[b, p % L] = x[b, i].to(cache.dtype)
        return cache
    for b in range(cache.shape[0]):
        p0 = int(pos[b])
        n = max(0, min(S, L - p0))
        if p0 >= 0 and n:
            if q8:
                cache[b, p0:p0 + n], scales[b, p0:p0 + n] = quantize_kv_rows(x[b, :n])
            else:
                cache[b, p0:p0 + n] = x[b, :n].to(cache.dtype)
    return cache


def _sdpa_ring_ref(q, kc, vc, pos, sc, window: int, limit: int, ct):
    """:func:`sdpa_cache_ref` over ring caches (dequantized already), a sequence at a time."""
    import torch

    B, Sq, H, D = q.shape
    C, G = kc.shape[1], H // kc.shape[2]
    out = torch.zeros(q.shape, dtype=ct)
    slots = torch.arange(C)
    for b in range(B):
        pb = int(pos[b])
        if pb < 0 or pb >= limit:   # a bad counter: no row sees anything
            continue
        pmax = pb + Sq - 1
        held = pmax - torch.remainder(pmax - slots, C)     # the position every slot holds after the step's writes
        qpos = pb + torch.arange(Sq).view(Sq, 1)
        keep = (held >= 0) & (held <= qpos) & (held > qpos - window)      # [Sq, C]
        seen = keep.any(dim=0)    # slots no row sees may hold anything (stale, never written): they are not read
        z = torch.zeros((), dtype=ct)
        kf = torch.where(seen.view(C, 1, 1), kc[b].to(ct), z).repeat_interleave(G, dim=1)
        vf = torch.where(seen.view(C, 1, 1), vc[b].to(ct), z).repeat_interleave(G, dim=1)
        s = torch.einsum("qhd,khd->hqk", q[b].to(ct), kf) * sc
        s = s.masked_fill(~keep[None], float("-inf"))
        p = torch.softmax(s, dim=-1)     # every row sees its own position (Sq <= C)
        out[b] = torch.einsum("hqk,khd->qhd", p, vf)
    return out.to(q.dtype)


def sdpa_cache_ref(q, kc, vc, pos, scale=None, kscales=None, vscales=None, window=None, limit=None):
    """Query i of sequence b at position pos[b] + i attends the cached keys
    0 .. min(pos[b] + i, L - 1) (fp32 math, fp64 for an fp64 q; grouped-query K / V heads).
    int8 caches with their scales: the attention of the values they hold (:func:`dequantize_kv_rows`).

    ``window`` and ``limit``: the caches are rings of C = L slots.  After the step's rows are written
    (:func:`kv_write_ref`) slot s holds position a(s) = pmax - ((pmax - s) mod C) for the step's last
    position pmax = pos[b] + Sq - 1; the query at qpos sees slot s iff 0 <= a(s) <= qpos and
    a(s) > qpos - window.  A counter outside [0, limit) gives zero rows."""
    import math

    import torch

    if (kc.dtype == torch.int8) != (kscales is not None) or (vc.dtype == torch.int8) != (vscales is not None):
        raise ValueError("sdpa_cache: int8 caches, and only int8 caches, take scales")
    if kscales is not None:
        kc, vc = dequantize_kv_rows(kc, kscales), dequantize_kv_rows(vc, vscales)

    B, Sq, H, D = q.shape
    L, Hkv = kc.shape[1], kc.shape[2]
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32   # an fp64 reference stays fp64
    if _ring_args("sdpa_cache", window, limit, L, Sq):
        return _sdpa_ring_ref(q, kc, vc, pos, scale if scale is not None else 1.0 / math.sqrt(D), window, limit, ct)
    kf = kc.to(ct).repeat_interleave(H // Hkv, dim=2)
    vf = vc.to(ct).repeat_interleave(H // Hkv, dim=2)
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    s = torch.einsum("bqhd,bkhd->bhqk", q.to(ct), kf) * sc
    qpos = pos.to(torch.long).view(B, 1) + torch.arange(Sq).view(1, Sq)            # [B, Sq]
    keep = torch.arange(L).view(1, 1, L) <= qpos.clamp(max=L - 1).view(B, Sq, 1)    # [B, Sq, L]
    s = s.masked_fill(~keep[:, None], float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhqk,bkhd->bqhd", p, vf).to(q.dtype)


def rotary_at_ref(x, cos, sin, pos):
    """rotate_half rotary of x [B, S, H, D] at positions pos[b] + i (table
    rows clamped to the table)."""
    import torch

    B, S, H, D = x.shape
    idx = (pos.to(torch.long).view(B, 1) + torch.arange(S).view(1, S)).clamp(0, cos.shape[0] - 1)   # [B, S]
    c = cos.float()[idx][:, :, None, :]
    sn = sin.float()[idx][:, :, None, :]
    xf = x.float()
    rot = torch.cat([-xf[..., D // 2:], xf[..., :D // 2]], dim=-1)
    return (xf * c + rot * sn).to(x.dtype)


def _pair2(attrs: dict, key: str, default: int) -> tuple[int, int]:
    v = attrs.get(key, default)
    return (v, v) if isinstance(v, int) else (v[0], v[1])


def _qkv_views(qkv, heads: int):
    """q, k, v [B, S, H, D] views of a fused projection [B, S, 3*H*D]."""
    B, S, n = qkv.shape
    return qkv.view(B, S, 3, heads, n // (3 * heads)).unbind(2)

