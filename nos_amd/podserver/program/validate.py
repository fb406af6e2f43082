"""Validation of a wire program: shape / dtype inference per op (with the
gfx950 kernels' constraints on a GPU), topological order and payload layout
-- everything is checked before a byte of device memory is allocated."""
from __future__ import annotations

import math

from .graph import Program
from .ir import (FLOAT_DTYPES, FORMAT, LORA_MAX_RANK, MOE_MAX_EXPERTS, MOE_MAX_TOP_K, MAX_NUMEL, MAX_PARAMS, MAX_NODES, MAX_RANK, MAX_STATE,
                 MAX_VARIANTS, MX4_BLOCK, OPS, PARAM_DTYPES, SPEC_CTL_WORDS, SPEC_MAX_K, SPEC_MIN_K, STATE_DTYPES, STATE_WRITERS, STOP_CTL_WORDS, ACTS,
                 BINARY, INTERP_MODES, UNARY, WIRE_DTYPES, Node, ProgramError, Value, _broadcast, _eps, _int, _name,
                 _pair, _req, _shape)


def _infer(node: Node, ins: list[Value], gpu: bool) -> tuple[tuple[int, ...], str]:
    """Output (shape, dtype) of a node; raises ProgramError on any mismatch,
    including the native kernels' constraints when the program runs on a GPU."""
    op, a = node.op, node.attrs
    what = f"node {node.output!r} ({op})"

    def arity(lo: int, hi: int) -> None:
        _req(lo <= len(ins) <= hi, f"{what}: takes {lo}..{hi} inputs, got {len(ins)}")

    def same_dtype() -> str:
        _req(len({v.dtype for v in ins}) == 1, f"{what}: inputs must share one dtype, got {[v.dtype for v in ins]}")
        return ins[0].dtype

    def only(*keys: str) -> None:
        extra = set(a) - set(keys)
        _req(not extra, f"{what}: unknown attributes {sorted(extra)}")

    if op == "linear":
        only("act")
        arity(2, 3)
        dt = same_dtype()
        x, w = ins[0], ins[1]
        _req(len(w.shape) == 2 and len(x.shape) >= 1 and x.shape[-1] == w.shape[1] and dt in FLOAT_DTYPES,
             f"{what}: float x [..., K] and weight [N, K] required, got {x.shape} and {w.shape}")
        if len(ins) == 3:
            _req(ins[2].shape == (w.shape[0],), f"{what}: bias must be [{w.shape[0]}], got {ins[2].shape}")
        _req(a.get("act") in ACTS, f"{what}: act must be one of {ACTS}")
        if gpu:
            k_mult = 64 if dt == "bf16" else 32
            _req(x.shape[-1] % k_mult == 0, f"{what}: the {dt} GEMM kernels need K % {k_mult} == 0, K = {x.shape[-1]}")
        return x.shape[:-1] + (w.shape[0],), dt
    if op == "linear_q8":
        # weight-only int8: wq [N, K] i8 with one fp32 scale per output row; fp32 x, bias and result
        only("act")
        arity(3, 4)
        x, w, sc = ins[0], ins[1], ins[2]
        _req(w.dtype == "i8" and w.kind == "param" and len(w.shape) == 2,
             f"{what}: the weight must be an i8 [N, K] param, got {w.kind} {w.dtype} {list(w.shape)}")
        _req(x.dtype == "fp32", f"{what}: x must be fp32 (int8 weights are an fp32 tenant's storage format; "
             f"a bf16 x is not taken), got {x.dtype}")
        _req(len(x.shape) >= 1 and x.shape[-1] == w.shape[1],
             f"{what}: x [..., K] and weight [N, K] required, got {x.shape} and {w.shape}")
        _req(sc.dtype == "fp32" and sc.shape == (w.shape[0],),
             f"{what}: wscale must be fp32 [{w.shape[0]}], got {sc.dtype} {list(sc.shape)}")
        if len(ins) == 4:
            _req(ins[3].dtype == "fp32" and ins[3].shape == (w.shape[0],),
                 f"{what}: bias must be fp32 [{w.shape[0]}], got {ins[3].dtype} {list(ins[3].shape)}")
        _req(a.get("act") in ACTS, f"{what}: act must be one of {ACTS}")
        if gpu:
            _req(x.shape[-1] % 32 == 0, f"{what}: the int8 GEMV and its h3 fallback need K % 32 == 0, "
                 f"K = {x.shape[-1]}")
        return x.shape[:-1] + (w.shape[0],), "fp32"
    if op == "linear_mx4":
        # weight-only MXFP4: codes [N, K / 2] u8 (two E2M1 elements a byte), scales [N, K / 32] u8 (E8M0)
        only("act")
        arity(3, 4)
        x, w, sc = ins[0], ins[1], ins[2]
        _req(w.dtype == "u8" and w.kind == "param" and len(w.shape) == 2,
             f"{what}: the weight must be a u8 [N, K / 2] param of MXFP4 codes, got {w.kind} {w.dtype} {list(w.shape)}")
        _req(x.dtype == "fp32", f"{what}: x must be fp32 (MXFP4 weights are an fp32 tenant's storage format; "
             f"a bf16 x is not taken), got {x.dtype}")
        K = x.shape[-1] if x.shape else 0
        _req(K > 0 and K % MX4_BLOCK == 0, f"{what}: K % {MX4_BLOCK} == 0 required (one scale byte per {MX4_BLOCK} "
             f"consecutive k), K = {K}")
        _req(w.shape[1] * 2 == K, f"{what}: x [..., K] and codes [N, K / 2] required, got {x.shape} and {w.shape}")
        _req(sc.dtype == "u8" and sc.kind == "param" and sc.shape == (w.shape[0], K // MX4_BLOCK),
             f"{what}: wscale must be a u8 [{w.shape[0]}, {K // MX4_BLOCK}] param (K / {MX4_BLOCK} block scales per "
             f"row), got {sc.kind} {sc.dtype} {list(sc.shape)}")
        if len(ins) == 4:
            _req(ins[3].dtype == "fp32" and ins[3].shape == (w.shape[0],),
                 f"{what}: bias must be fp32 [{w.shape[0]}], got {ins[3].dtype} {list(ins[3].shape)}")
        _req(a.get("act") in ACTS, f"{what}: act must be one of {ACTS}")
        return x.shape[:-1] + (w.shape[0],), "fp32"
    if op == "layernorm":
        only("eps")
        arity(3, 3)
        dt = same_dtype()
        d = ins[0].shape[-1] if ins[0].shape else 0
        _req(ins[1].shape == (d,) and ins[2].shape == (d,) and dt in FLOAT_DTYPES, f"{what}: gamma/beta must be [{d}]")
        eps = a.get("eps", 1e-5)
        _req(isinstance(eps, (int, float)) and 0 < eps < 1, f"{what}: eps must be in (0, 1)")
        return ins[0].shape, dt
    if op == "attention":
        only("heads", "scale", "causal")
        arity(1, 1)
        x = ins[0]
        h = _int(a.get("heads"), f"{what}: heads", 1)
        _req(len(x.shape) == 3 and x.shape[2] % (3 * h) == 0 and x.dtype in FLOAT_DTYPES,
             f"{what}: qkv must be a float [B, S, 3*heads*D], got {x.shape} with {h} heads")
        d = x.shape[2] // (3 * h)
        if "scale" in a:
            _req(isinstance(a["scale"], (int, float)) and a["scale"] > 0, f"{what}: scale must be > 0")
        _req(isinstance(a.get("causal", False), bool), f"{what}: causal must be a bool")
        if gpu:
            _req(d in (64, 128), f"{what}: the attention kernels take head_dim 64 or 128, got {d}")
        return (x.shape[0], x.shape[1], h * d), x.dtype
    if op in BINARY:
        only()
        arity(2, 2)
        dt = same_dtype()
        _req(dt in FLOAT_DTYPES, f"{what}: takes float tensors")
        return _broadcast(ins[0].shape, ins[1].shape, what), dt
    if op in UNARY:
        only()
        arity(1, 1)
        _req(ins[0].dtype in FLOAT_DTYPES, f"{what}: takes a float tensor")
        return ins[0].shape, ins[0].dtype
    if op == "cat":
        only("dim")
        arity(1, 64)
        dt = same_dtype()
        r = len(ins[0].shape)
        dim = _int(a.get("dim"), f"{what}: dim")
        dim = dim + r if dim < 0 else dim
        _req(0 <= dim < r, f"{what}: dim out of range")
        for v in ins[1:]:
            _req(len(v.shape) == r and all(v.shape[i] == ins[0].shape[i] for i in range(r) if i != dim),
                 f"{what}: shapes {[v.shape for v in ins]} differ outside dim {dim}")
        s = list(ins[0].shape)
        s[dim] = sum(v.shape[dim] for v in ins)
        return tuple(s), dt
    if op == "slice":
        only("dim", "start", "end")
        arity(1, 1)
        s = list(ins[0].shape)
        dim = _int(a.get("dim"), f"{what}: dim")
        dim = dim + len(s) if dim < 0 else dim
        _req(0 <= dim < len(s), f"{what}: dim out of range")
        start, end = _int(a.get("start"), f"{what}: start", 0), _int(a.get("end"), f"{what}: end", 1)
        _req(start < end <= s[dim], f"{what}: need 0 <= start < end <= {s[dim]}, got {start}:{end}")
        s[dim] = end - start
        return tuple(s), ins[0].dtype
    if op == "reshape":
        only("shape")
        arity(1, 1)
        want = a.get("shape")
        _req(isinstance(want, list) and len(want) <= MAX_RANK and all(isinstance(d, int) for d in want),
             f"{what}: shape must be a list of integers")
        _req(sum(1 for d in want if d == -1) <= 1 and all(d == -1 or d >= 1 for d in want),
             f"{what}: shape dims must be >= 1, at most one -1")
        _req(all(d <= MAX_NUMEL for d in want), f"{what}: shape dims must be <= {MAX_NUMEL}")
        n = ins[0].numel
        known = math.prod(d for d in want if d != -1)
        if -1 in want:
            _req(known > 0 and n % known == 0, f"{what}: cannot reshape {ins[0].shape} to {want}")
            want = [n // known if d == -1 else d for d in want]
        _req(math.prod(want) == n, f"{what}: cannot reshape {ins[0].shape} to {want}")
        return tuple(want), ins[0].dtype
    if op == "permute":
        only("dims")
        arity(1, 1)
        dims = a.get("dims")
        _req(isinstance(dims, list) and all(isinstance(d, int) and not isinstance(d, bool) for d in dims)
             and sorted(dims) == list(range(len(ins[0].shape))),
             f"{what}: dims must be a permutation of 0..{len(ins[0].shape) - 1}")
        return tuple(ins[0].shape[d] for d in dims), ins[0].dtype
    if op == "expand":
        only("shape")
        arity(1, 1)
        want = a.get("shape")
        s = ins[0].shape
        _req(isinstance(want, list) and len(want) == len(s), f"{what}: shape must have rank {len(s)}")
        out = []
        for src, d in zip(s, want):
            _req(isinstance(d, int) and (d == -1 or d == src or (src == 1 and 1 <= d <= MAX_NUMEL)),
                 f"{what}: cannot expand {s} to {want}")
            out.append(src if d == -1 else d)
        return tuple(out), ins[0].dtype
    if op == "cast":
        only("dtype")
        arity(1, 1)
        _req(a.get("dtype") in FLOAT_DTYPES and ins[0].dtype in FLOAT_DTYPES,
             f"{what}: casts between {FLOAT_DTYPES} only")
        return ins[0].shape, a["dtype"]
    if op == "interpolate":
        only("size", "mode")
        arity(1, 1)
        x = ins[0]
        _req(len(x.shape) == 4 and x.dtype == "fp32", f"{what}: takes an fp32 [N, C, H, W] tensor")
        size = a.get("size")
        _req(isinstance(size, list) and len(size) == 2 and all(isinstance(d, int) and 1 <= d <= 65536 for d in size),
             f"{what}: size must be [H, W]")
        _req(a.get("mode", "bicubic") in INTERP_MODES, f"{what}: mode must be one of {INTERP_MODES}")
        return (x.shape[0], x.shape[1], size[0], size[1]), x.dtype
    if op == "conv2d":
        only("stride", "padding", "dilation", "groups")
        arity(2, 3)
        dt = same_dtype()
        x, w = ins[0], ins[1]
        g = a.get("groups", 1)
        _req(isinstance(g, int) and not isinstance(g, bool) and 1 <= g <= 65536, f"{what}: groups must be an int >= 1")
        _req(len(x.shape) == 4 and len(w.shape) == 4 and x.shape[1] == w.shape[1] * g and w.shape[0] % g == 0,
             f"{what}: x [N, C, H, W] and weight [OC, C / groups, KH, KW] (OC % groups == 0) required, got "
             f"{x.shape} and {w.shape} for groups = {g}")
        if len(ins) == 3:
            _req(ins[2].shape == (w.shape[0],), f"{what}: bias must be [{w.shape[0]}]")
        st = _pair(a.get("stride", [1, 1]), f"{what}: stride", 1)
        pd = _pair(a.get("padding", [0, 0]), f"{what}: padding", 0)
        dl = _pair(a.get("dilation", [1, 1]), f"{what}: dilation", 1)
        oh = (x.shape[2] + 2 * pd[0] - dl[0] * (w.shape[2] - 1) - 1) // st[0] + 1
        ow = (x.shape[3] + 2 * pd[1] - dl[1] * (w.shape[3] - 1) - 1) // st[1] + 1
        _req(oh >= 1 and ow >= 1, f"{what}: empty output for input {x.shape}")
        return (x.shape[0], w.shape[0], oh, ow), dt
    if op == "batchnorm":
        only("eps")
        arity(5, 5)
        dt = same_dtype()
        x = ins[0]
        _req(len(x.shape) >= 2 and all(v.shape == (x.shape[1],) for v in ins[1:]),
             f"{what}: x [N, C, ...] and gamma / beta / mean / var [C] required")
        _eps(a, what)
        return x.shape, dt
    if op in ("max_pool2d", "avg_pool2d"):
        only("kernel", "stride", "padding")
        arity(1, 1)
        x = ins[0]
        _req(len(x.shape) == 4 and x.dtype in FLOAT_DTYPES, f"{what}: takes a float [N, C, H, W] tensor")
        k = _pair(a.get("kernel"), f"{what}: kernel", 1)
        st = _pair(a.get("stride", list(k)), f"{what}: stride", 1)
        pd = _pair(a.get("padding", [0, 0]), f"{what}: padding", 0)
        _req(pd[0] <= k[0] // 2 and pd[1] <= k[1] // 2, f"{what}: padding must be <= kernel / 2")
        oh, ow = (x.shape[2] + 2 * pd[0] - k[0]) // st[0] + 1, (x.shape[3] + 2 * pd[1] - k[1]) // st[1] + 1
        _req(oh >= 1 and ow >= 1, f"{what}: empty output")
        return (x.shape[0], x.shape[1], oh, ow), x.dtype
    if op in ("mean", "sum"):
        only("dims", "keepdim")
        arity(1, 1)
        x = ins[0]
        r = len(x.shape)
        dims = a.get("dims")
        _req(isinstance(dims, list) and dims and all(isinstance(d, int) and not isinstance(d, bool) and -r <= d < r
                                                      for d in dims), f"{what}: dims must be a list of axes")
        dd = sorted({d % r for d in dims})
        keep = a.get("keepdim", False)
        _req(isinstance(keep, bool), f"{what}: keepdim must be a bool")
        _req(x.dtype in FLOAT_DTYPES, f"{what}: takes a float tensor")
        return tuple((1 if i in dd else n) for i, n in enumerate(x.shape) if keep or i not in dd), x.dtype
    if op == "matmul":
        only()
        arity(2, 2)
        dt = same_dtype()
        x, y = ins
        _req(len(x.shape) >= 2 and len(y.shape) >= 2 and x.shape[-1] == y.shape[-2],
             f"{what}: [..., M, K] @ [..., K, N] required, got {x.shape} and {y.shape}")
        bx, by = x.shape[:-2], y.shape[:-2]
        _req(not bx or not by or bx == by, f"{what}: batch dims must match or one side be 2-D")
        return (bx or by) + (x.shape[-2], y.shape[-1]), dt
    if op == "softmax":
        only("dim")
        arity(1, 1)
        _req(a.get("dim", -1) in (-1, len(ins[0].shape) - 1), f"{what}: softmax runs over the last dim")
        _req(ins[0].dtype in FLOAT_DTYPES, f"{what}: takes a float tensor")
        return ins[0].shape, ins[0].dtype
    if op == "embedding":
        only()
        arity(2, 2)
        ids, table = ins
        _req(ids.dtype == "i32", f"{what}: ids must be i32, got {ids.dtype}")
        _req(len(table.shape) == 2 and table.dtype in FLOAT_DTYPES, f"{what}: table must be a float [V, D]")
        if gpu:
            _req(table.shape[1] * WIRE_DTYPES[table.dtype] % 16 == 0, f"{what}: table rows must be 16-byte multiples")
        return ids.shape + (table.shape[1],), table.dtype
    if op == "rmsnorm":
        only("eps")
        arity(2, 2)
        dt = same_dtype()
        _req(len(ins[0].shape) >= 1 and ins[1].shape == (ins[0].shape[-1],), f"{what}: weight must be [D]")
        _eps(a, what)
        return ins[0].shape, dt
    if op == "rotary":
        only()
        arity(3, 3)
        x, c, sn = ins
        _req(len(x.shape) == 4 and x.shape[3] % 2 == 0 and x.dtype in FLOAT_DTYPES,
             f"{what}: x must be [B, S, H, D] with D even")
        _req(c.shape == sn.shape == (x.shape[1], x.shape[3]) and c.dtype == sn.dtype == "fp32",
             f"{what}: cos / sin must be fp32 [S, D] = [{x.shape[1]}, {x.shape[3]}]")
        return x.shape, x.dtype
    if op == "sdpa":
        only("causal", "scale")
        arity(3, 3)
        dt = same_dtype()
        q, k, v = ins
        _req(len(q.shape) == 4 and len(k.shape) == 4 and k.shape == v.shape and q.shape[0] == k.shape[0]
             and q.shape[3] == k.shape[3] and q.shape[2] % k.shape[2] == 0,
             f"{what}: q [B, Sq, H, D], k / v [B, Skv, Hkv, D] with H % Hkv == 0 required, got {q.shape}, {k.shape}")
        _req(isinstance(a.get("causal", False), bool), f"{what}: causal must be a bool")
        if a.get("causal"):
            _req(q.shape[1] <= k.shape[1], f"{what}: causal attention needs Sq <= Skv")
        if "scale" in a:
            _req(isinstance(a["scale"], (int, float)) and a["scale"] > 0, f"{what}: scale must be > 0")
        if gpu:
            _req(q.shape[3] in (64, 128), f"{what}: the attention kernels take head_dim 64 or 128, got {q.shape[3]}")
        return q.shape, dt
    if op == "kv_write":
        # cache [B, L, Hkv, D] <- x [B, S, Hkv, D] at rows pos[b] .. pos[b] + S - 1 (rows past L are dropped)
        # an i8 cache (rows quantized as they are written) takes its fp32 scales state [B, L, Hkv] as input 3
        # window + limit: the cache is a ring of C = L slots (position p in slot p % C, rows at p >= limit dropped)
        only("window", "limit")
        arity(3, 4)
        c, x, p = ins[:3]
        _req(len(c.shape) == 4 and c.dtype in FLOAT_DTYPES + ("i8",),
             f"{what}: the cache must be a float or i8 [B, L, Hkv, D] state")
        if len(x.shape) == 4:
            _ring_attrs(a, c.shape[1], x.shape[1], what)
        q8 = c.dtype == "i8"
        _req(q8 or len(ins) == 3, f"{what}: a {c.dtype} cache takes no scales (input 3 belongs to an i8 cache)")
        _req(not q8 or len(ins) == 4, f"{what}: an i8 cache needs its scales state as input 3")
        xdt = "fp32" if q8 else c.dtype
        _req(len(x.shape) == 4 and x.shape[0] == c.shape[0] and x.shape[2:] == c.shape[2:] and x.dtype == xdt
             and x.shape[1] <= c.shape[1], f"{what}: x must be [{c.shape[0]}, S <= {c.shape[1]}, {c.shape[2]}, "
             f"{c.shape[3]}] {xdt}, got {x.shape} {x.dtype}")
        _pos_vector(p, c.shape[0], what)
        if q8:
            _scales_state(ins[3], c, what)
        return c.shape, c.dtype
    if op == "sdpa_cache":
        # q [B, Sq, H, D] at positions pos[b] + i over the cached keys 0 .. pos[b] + i (causal)
        # i8 caches take their fp32 scales states [B, L, Hkv] as inputs 4 (K) and 5 (V)
        # window + limit: ring caches; the query at p attends the positions max(0, p - window + 1) .. p
        only("scale", "window", "limit")
        _req(len(ins) in (4, 6), f"{what}: takes 4 inputs (6 with the scales of i8 caches), got {len(ins)}")
        q, kc, vc, p = ins[:4]
        if len(q.shape) == 4 and len(kc.shape) == 4:
            _ring_attrs(a, kc.shape[1], q.shape[1], what)
        _req(len(q.shape) == 4 and len(kc.shape) == 4 and kc.shape == vc.shape and kc.dtype == vc.dtype
             and q.shape[0] == kc.shape[0] and q.shape[3] == kc.shape[3] and q.shape[2] % kc.shape[2] == 0
             and q.shape[1] <= kc.shape[1] and q.dtype in FLOAT_DTYPES and kc.dtype in FLOAT_DTYPES + ("i8",),
             f"{what}: q [B, Sq, H, D], caches [B, L >= Sq, Hkv, D] with H % Hkv == 0 required, got {q.shape}, "
             f"{kc.shape}")
        q8 = kc.dtype == "i8"
        _req(q8 or len(ins) == 4, f"{what}: {kc.dtype} caches take no scales (inputs 4 and 5 belong to i8 caches)")
        _req(not q8 or len(ins) == 6, f"{what}: i8 caches need their scales states as inputs 4 and 5")
        if q8:
            _req(q.dtype == "fp32", f"{what}: q must be fp32 over i8 caches (they are an fp32 tenant's storage "
                 f"format), got {q.dtype}")
            _scales_state(ins[4], kc, what)
            _scales_state(ins[5], vc, what)
        _pos_vector(p, q.shape[0], what)
        if "scale" in a:
            _req(isinstance(a["scale"], (int, float)) and not isinstance(a["scale"], bool) and a["scale"] > 0,
                 f"{what}: scale must be > 0")
        if gpu:
            _req(q.shape[3] in (64, 128), f"{what}: the decode attention kernel takes head_dim 64 or 128")
            _req(q.shape[2] // kc.shape[2] <= 16, f"{what}: at most 16 query heads per K / V head")
        return q.shape, q.dtype
    if op == "rotary_at":
        only()
        arity(4, 4)
        x, c, sn, p = ins
        _req(len(x.shape) == 4 and x.shape[3] % 2 == 0 and x.dtype in FLOAT_DTYPES,
             f"{what}: x must be [B, S, H, D] with D even")
        _req(len(c.shape) == 2 and c.shape == sn.shape and c.shape[1] == x.shape[3] and c.dtype == sn.dtype == "fp32",
             f"{what}: cos / sin must be fp32 [positions, {x.shape[3]}]")
        _pos_vector(p, x.shape[0], what)
        return x.shape, x.dtype
    if op in ("pos_add", "pos_set"):
        only("n" if op == "pos_add" else "value")
        arity(1, 2 if op == "pos_add" else 1)
        _req(ins[0].dtype == "i32" and len(ins[0].shape) == 1, f"{what}: takes an i32 [B] position state")
        if len(ins) == 2:   # a stopping tenant's: rows whose done flag is set keep their counter
            _done_vector(ins[1], ins[0].shape[0], what)
        v = a.get("n" if op == "pos_add" else "value")
        _req(isinstance(v, int) and not isinstance(v, bool) and 0 <= v <= 1 << 24,
             f"{what}: {'n' if op == 'pos_add' else 'value'} must be an int in [0, 2^24]")
        return ins[0].shape, "i32"
    if op == "argmax":
        only("dim")
        arity(1, 1)
        _req(a.get("dim", -1) in (-1, len(ins[0].shape) - 1) and len(ins[0].shape) >= 1,
             f"{what}: argmax runs over the last dim")
        _req(ins[0].dtype in FLOAT_DTYPES, f"{what}: takes a float tensor")
        return ins[0].shape[:-1], "i32"
    if op == "sample":
        # one token per row of logits, drawn as the tenant's control words say (ops.tenant.sample);
        # pos keys the draw and is only read
        only()
        arity(3, 3)
        x, ctl, p = ins
        _req(len(x.shape) >= 1 and x.dtype in FLOAT_DTYPES, f"{what}: takes a float tensor (last dim: the logits)")
        _req(ctl.kind == "state" and ctl.dtype == "i32" and ctl.shape == (4,),
             f"{what}: the control words must be an i32 [4] state, got {ctl.kind} {ctl.name!r} {ctl.dtype} "
             f"{list(ctl.shape)}")
        _pos_vector(p, math.prod(x.shape[:-1]), what)
        return x.shape[:-1], "i32"
    if op == "seen_mark":
        # seen [B, W] (i32 bitmaps: bit id & 31 of word id >> 5) |= the ids [B, S]; reset: cleared first
        only("reset")
        arity(2, 2)
        seen, ids = ins
        _req(seen.dtype == "i32" and len(seen.shape) == 2, f"{what}: seen must be an i32 [B, words] bitmap state, "
             f"got {seen.dtype} {list(seen.shape)}")
        _req(ids.dtype == "i32" and len(ids.shape) == 2 and ids.shape[0] == seen.shape[0],
             f"{what}: ids must be i32 [{seen.shape[0]}, S], got {ids.dtype} {list(ids.shape)}")
        _req(isinstance(a.get("reset", False), bool), f"{what}: reset must be a bool")
        return seen.shape, "i32"
    if op == "penalize":
        # the logits of the tokens in seen under the control words' repetition penalty (ops.tenant.penalize)
        only()
        arity(3, 3)
        x, seen, ctl = ins
        _req(len(x.shape) >= 1 and x.dtype in FLOAT_DTYPES, f"{what}: takes a float tensor (last dim: the logits)")
        rows, words = math.prod(x.shape[:-1]), -(-x.shape[-1] // 32)
        _req(seen.dtype == "i32" and seen.shape == (rows, words),
             f"{what}: seen must be an i32 [{rows}, {words}] bitmap (one bit per logit, 32 a word), got "
             f"{seen.dtype} {list(seen.shape)}")
        _stop_ctl(ctl, what)
        if gpu:
            _req(rows <= 65535, f"{what}: at most 65535 rows of logits")
        return x.shape, x.dtype
    if op == "stop_ids":
        # done[b] ? pad_id : next_ids[b]
        only()
        arity(3, 3)
        nxt, done, ctl = ins
        _req(nxt.dtype == "i32", f"{what}: next ids must be i32, got {nxt.dtype}")
        _done_vector(done, nxt.numel, what)
        _stop_ctl(ctl, what)
        return nxt.shape, "i32"
    if op == "done_mark":
        # done[b] |= ids[b] is one of the control words' stop ids
        only()
        arity(3, 3)
        done, ids, ctl = ins
        _req(ids.dtype == "i32", f"{what}: ids must be i32, got {ids.dtype}")
        _done_vector(done, ids.numel, what)
        _stop_ctl(ctl, what)
        return done.shape, "i32"
    if op == "hist_write":
        # hist [B, L] <- ids[:, :lead] then tail (with n: its first n[b] columns; nothing for n[b] = 0)
        # from position pos[b] - back on; indices outside [0, L) are dropped
        only("back", "lead")
        arity(3, 5)
        hist, p, ids = ins[:3]
        _hist_state(hist, what)
        _pos_vector(p, hist.shape[0], what)
        for v, name in zip(ins[2:4], ("ids", "tail")):
            _req(v.dtype == "i32" and len(v.shape) == 2 and v.shape[0] == hist.shape[0],
                 f"{what}: {name} must be i32 [{hist.shape[0]}, S], got {v.dtype} {list(v.shape)}")
        if len(ins) == 5:
            _req(ins[4].dtype == "i32" and ins[4].shape == (hist.shape[0],),
                 f"{what}: n must be an i32 [{hist.shape[0]}] (a count per row), got {ins[4].dtype} {list(ins[4].shape)}")
        back, lead = a.get("back", 0), a.get("lead", ids.shape[1])
        _req(isinstance(back, int) and not isinstance(back, bool) and 0 <= back <= 1 << 24,
             f"{what}: back must be an int in [0, 2^24]")
        _req(isinstance(lead, int) and not isinstance(lead, bool) and 0 <= lead <= ids.shape[1],
             f"{what}: lead must be an int in [0, {ids.shape[1]}] (ids' columns)")
        return hist.shape, "i32"
    if op == "spec_accept":
        # a verify step's advance per row (ops.tenant.spec_accept): ids and the drawn g [B, K], pos, ctl
        only("limit")
        arity(4, 4)
        ids, g, p, ctl = ins
        _req(ids.dtype == g.dtype == "i32" and len(ids.shape) == 2 and ids.shape == g.shape
             and SPEC_MIN_K <= ids.shape[1] <= SPEC_MAX_K,
             f"{what}: ids and the drawn ids must both be i32 [B, {SPEC_MIN_K} <= K <= {SPEC_MAX_K}], got "
             f"{ids.dtype} {list(ids.shape)} and {g.dtype} {list(g.shape)}")
        _pos_vector(p, ids.shape[0], what)
        _req(ctl.kind == "state" and ctl.dtype == "i32" and ctl.shape == (SPEC_CTL_WORDS,),
             f"{what}: the speculation control words must be an i32 [{SPEC_CTL_WORDS}] state, got {ctl.kind} "
             f"{ctl.name!r} {ctl.dtype} {list(ctl.shape)}")
        _int(a.get("limit"), f"{what}: limit", 1)
        return (ids.shape[0],), "i32"
    if op == "pos_advance":
        only()
        arity(2, 2)
        _req(ins[0].dtype == "i32" and len(ins[0].shape) == 1, f"{what}: takes an i32 [B] position state")
        _req(ins[1].dtype == "i32" and ins[1].shape == ins[0].shape,
             f"{what}: the advance must be an i32 {list(ins[0].shape)}, got {ins[1].dtype} {list(ins[1].shape)}")
        return ins[0].shape, "i32"
    if op == "spec_draft":
        only("k")
        arity(2, 2)
        _hist_state(ins[0], what)
        _pos_vector(ins[1], ins[0].shape[0], what)
        k = _int(a.get("k"), f"{what}: k", SPEC_MIN_K)
        _req(k <= SPEC_MAX_K, f"{what}: k must be <= {SPEC_MAX_K}")
        return (ins[0].shape[0], k), "i32"
    if op == "lora":
        # the low-rank delta of the adapter each sequence's sel names: (x[b] @ A[a - 1].T) @ B[a - 1].T for
        # a = sel[b] in [1, n], zeros otherwise (ops.tenant.lora_ref); added to a linear's output
        only()
        arity(4, 4)
        x, A, B, sel = ins
        _req(x.dtype == "fp32" and len(x.shape) == 3,
             f"{what}: x must be fp32 [batch, S, K] (adapters are an fp32 tenant's; a bf16 x is not taken), got "
             f"{x.dtype} {list(x.shape)}")
        _req(sel.kind == "state", f"{what}: sel must be a state (the program's adapter state, which the server "
             f"fills per request), got {sel.kind} {sel.name!r}")
        _req(sel.dtype == "i32" and sel.shape == (x.shape[0],),
             f"{what}: sel must be an i32 [{x.shape[0]}] state (an adapter per sequence), got {sel.dtype} "
             f"{list(sel.shape)}")
        _req(A.kind == B.kind == "param" and A.dtype == B.dtype == "fp32" and len(A.shape) == len(B.shape) == 3,
             f"{what}: A [n, R, K] and B [n, N, R] must be fp32 params, got {A.kind} {A.dtype} {list(A.shape)} and "
             f"{B.kind} {B.dtype} {list(B.shape)}")
        _req(A.shape[0] == B.shape[0], f"{what}: A and B must hold the same number of adapters n, got "
             f"{A.shape[0]} and {B.shape[0]}")
        _req(A.shape[1] == B.shape[2], f"{what}: A [n, R, K] and B [n, N, R] must share the rank R, got "
             f"{A.shape[1]} and {B.shape[2]}")
        _req(A.shape[2] == x.shape[2], f"{what}: A [n, R, K] must have x's K = {x.shape[2]}, got {A.shape[2]}")
        if gpu:
            _req(A.shape[1] % 4 == 0 and A.shape[1] <= LORA_MAX_RANK and x.shape[2] % 4 == 0,
                 f"{what}: the adapter kernels take a rank R <= {LORA_MAX_RANK} with R % 4 == 0 and K % 4 == 0, got "
                 f"R = {A.shape[1]}, K = {x.shape[2]}")
        return (x.shape[0], x.shape[1], B.shape[1]), "fp32"
    if op == "moe":
        # a sparse mixture-of-experts MLP (transformers' MixtralSparseMoeBlock; ops.tenant.moe_ref): per row the
        # router's softmax over E experts, the top_k largest renormalised, and their SwiGLU MLPs weighted
        only("top_k")
        arity(4, 4)
        x, Wr, W13, W2 = ins
        _req(x.dtype == "fp32" and len(x.shape) >= 2,
             f"{what}: x must be fp32 [..., H] (a bf16 x is not taken), got {x.dtype} {list(x.shape)}")
        _req(all(w.kind == "param" and w.dtype == "fp32" for w in (Wr, W13, W2)),
             f"{what}: Wr, W13 and W2 must be fp32 params (the weights are chosen on the device, never computed), got "
             + ", ".join(f"{w.kind} {w.dtype} {w.name!r}" for w in (Wr, W13, W2)))
        H = x.shape[-1]
        _req(len(Wr.shape) == 2 and len(W13.shape) == 3 and len(W2.shape) == 3 and W13.shape[1] % 2 == 0
             and Wr.shape == (W13.shape[0], H) and W13.shape[2] == H
             and W2.shape == (W13.shape[0], H, W13.shape[1] // 2),
             f"{what}: the weights' shapes must match: Wr [E, H], W13 [E, 2I, H] and W2 [E, H, I] with H = {H}, got "
             f"{list(Wr.shape)}, {list(W13.shape)} and {list(W2.shape)}")
        E, I = Wr.shape[0], W13.shape[1] // 2
        _req(E <= MOE_MAX_EXPERTS, f"{what}: E = {E} experts; E <= {MOE_MAX_EXPERTS} required")
        k = _int(a.get("top_k"), f"{what}: top_k", 1)
        _req(k <= min(E, MOE_MAX_TOP_K), f"{what}: 1 <= top_k <= min(E, {MOE_MAX_TOP_K}) = {min(E, MOE_MAX_TOP_K)} "
             f"required, got {k}")
        _req(H % 4 == 0 and I % 4 == 0, f"{what}: H % 4 == 0 and I % 4 == 0 required (16-byte loads), got H = {H}, "
             f"I = {I}")
        return x.shape, "fp32"
    if op in ("moe_q8", "moe_mx4"):
        # moe over quantized experts (ops.tenant.moe_q8_ref / moe_mx4_ref): what moe checks, and the storage format's
        # params -- int8 codes [E, N, K] with fp32 scales [E, N], or MXFP4 codes u8 [E, N, K / 2] with E8M0 scale
        # bytes u8 [E, N, K / 32]; the router stays an fp32 param
        only("top_k")
        arity(6, 6)
        x, Wr, W13, S13, W2, S2 = ins
        q8 = op == "moe_q8"
        fmt, cdt, sdt, mult, per = ("int8", "i8", "fp32", 16, 1) if q8 else ("MXFP4", "u8", "u8", MX4_BLOCK, 2)
        _req(x.dtype == "fp32" and len(x.shape) >= 2,
             f"{what}: x must be fp32 [..., H] (a bf16 x is not taken), got {x.dtype} {list(x.shape)}")
        _req(Wr.kind == "param" and Wr.dtype == "fp32",
             f"{what}: the router Wr must be an fp32 param (routing is not quantized), got {Wr.kind} {Wr.dtype} "
             f"{Wr.name!r}")
        _req(all(w.kind == "param" and w.dtype == cdt for w in (W13, W2)),
             f"{what}: the expert codes W13 and W2 must be {cdt} params ({fmt} is a storage format: the weights are "
             f"chosen on the device, never computed), got "
             + ", ".join(f"{w.kind} {w.dtype} {w.name!r}" for w in (W13, W2)))
        _req(all(w.kind == "param" and w.dtype == sdt for w in (S13, S2)),
             f"{what}: the expert scales must be {sdt} params, got "
             + ", ".join(f"{w.kind} {w.dtype} {w.name!r}" for w in (S13, S2)))
        H = x.shape[-1]
        _req(len(Wr.shape) == 2 and len(W13.shape) == 3 and len(W2.shape) == 3 and W13.shape[1] % 2 == 0
             and H % per == 0 and Wr.shape == (W13.shape[0], H) and W13.shape[2] * per == H
             and W2.shape[:2] == (W13.shape[0], H) and W2.shape[2] * per == W13.shape[1] // 2,
             f"{what}: the weights' shapes must match: Wr [E, H], codes [E, 2I, H{' / 2' if per == 2 else ''}] and "
             f"[E, H, I{' / 2' if per == 2 else ''}] with H = {H}, got {list(Wr.shape)}, {list(W13.shape)} and "
             f"{list(W2.shape)}")
        E, I = Wr.shape[0], W13.shape[1] // 2
        _req(H % mult == 0 and I % mult == 0,
             f"{what}: H % {mult} == 0 and I % {mult} == 0 required ("
             + ("16 int8 weights a 16-byte load" if q8 else f"an MXFP4 block is {MX4_BLOCK} consecutive inputs under one "
                "scale byte") + f"), got H = {H}, I = {I}")
        want13, want2 = ((E, 2 * I), (E, H)) if q8 else ((E, 2 * I, H // MX4_BLOCK), (E, H, I // MX4_BLOCK))
        _req(S13.shape == want13 and S2.shape == want2,
             f"{what}: the scales' shapes must match the codes: {list(want13)} and {list(want2)} ("
             + ("one per row" if q8 else f"one byte per {MX4_BLOCK} inputs of a row")
             + f"), got {list(S13.shape)} and {list(S2.shape)}")
        _req(E <= MOE_MAX_EXPERTS, f"{what}: E = {E} experts; E <= {MOE_MAX_EXPERTS} required")
        k = _int(a.get("top_k"), f"{what}: top_k", 1)
        _req(k <= min(E, MOE_MAX_TOP_K), f"{what}: 1 <= top_k <= min(E, {MOE_MAX_TOP_K}) = {min(E, MOE_MAX_TOP_K)} "
             f"required, got {k}")
        return x.shape, "fp32"
    raise ProgramError(f"{what}: op {op!r} is not one the pod server runs (whitelist: {' '.join(OPS)})")


def _hist_state(h: Value, what: str) -> None:
    _req(h.dtype == "i32" and len(h.shape) == 2 and h.shape[1] <= 1 << 28,
         f"{what}: hist must be an i32 [B, L <= 2^28] state (the rows' token history), got {h.dtype} {list(h.shape)}")


def _pos_vector(p: Value, b: int, what: str) -> None:
    _req(p.dtype == "i32" and p.shape == (b,), f"{what}: pos must be an i32 [{b}] (a position state), got {p.shape}")


def _done_vector(d: Value, b: int, what: str) -> None:
    _req(d.dtype == "i32" and d.shape == (b,), f"{what}: done must be an i32 [{b}] (a flag per row), got "
         f"{d.dtype} {list(d.shape)}")


def _stop_ctl(ctl: Value, what: str) -> None:
    """The stopping control words: an i32 [8] STATE (the server fills it per request)."""
    _req(ctl.kind == "state" and ctl.dtype == "i32" and ctl.shape == (STOP_CTL_WORDS,),
         f"{what}: the stopping control words must be an i32 [{STOP_CTL_WORDS}] state, got {ctl.kind} {ctl.name!r} "
         f"{ctl.dtype} {list(ctl.shape)}")


def _ring_name(ring: tuple | None) -> str:
    return "a plain cache" if ring is None else f"a ring of window {ring[0]} and limit {ring[1]}"


def _scales_state(s: Value, cache: Value, what: str) -> None:
    """The row scales of an i8 cache [B, L, Hkv, D]: an fp32 [B, L, Hkv] state."""
    _req(s.kind == "state" and s.dtype == "fp32" and s.shape == cache.shape[:3],
         f"{what}: the scales of an i8 cache must be an fp32 {list(cache.shape[:3])} state, got {s.kind} "
         f"{s.name!r} {s.dtype} {list(s.shape)}")


def _ring_attrs(a: dict, C: int, S: int, what: str) -> None:
    """``window`` / ``limit`` of a ``kv_write`` / ``sdpa_cache`` over a ring cache of C slots, at a step of S rows:
    the step writes its rows and then attends, so the ring holds the first row's window and the whole step."""
    _req(("window" in a) == ("limit" in a), f"{what}: window and limit are given together (a ring cache), or neither")
    if "window" not in a:
        return
    for k in ("window", "limit"):
        _req(isinstance(a[k], int) and not isinstance(a[k], bool) and 1 <= a[k] <= 1 << 30,
             f"{what}: {k} must be an int >= 1, got {a[k]!r}")
    W, limit = a["window"], a["limit"]
    _req(C <= limit, f"{what}: a ring cache of {C} slots is longer than its limit {limit}")
    _req(C >= min(limit, W + S - 1), f"{what}: a ring cache needs min(limit, window + S - 1) = "
         f"{min(limit, W + S - 1)} slots for window {W} and {S} rows a step, the cache has {C}")


# the slots an i8 state (a quantized cache) and its scales state may fill
_Q8_CACHE_SLOTS = {"kv_write": {0: 3}, "sdpa_cache": {1: 4, 2: 5}}   # op -> {cache slot: its scales' slot}


# the states a stopping program's ops name: op -> ((role, input slot), ...); a program has one of each
_STOP_ROLES = {"seen_mark": (("seen", 0),), "penalize": (("seen", 1), ("stopping", 2)),
               "stop_ids": (("done", 1), ("stopping", 2)), "done_mark": (("done", 0), ("stopping", 2)),
               "pos_add": (("done", 1),),   # the mask of pos_add(pos, done): the flags stop_ids / done_mark name
               # a speculating program's: the token history and the control words (the budget's end)
               "hist_write": (("hist", 0),), "spec_draft": (("hist", 0),), "spec_accept": (("speculate", 3),)}


def parse_variants(objs: list, payload: bytes | memoryview = b"", gpu: bool = False) -> list[Program]:
    """A tenant's programs for several input shapes (sequence-length or image
    size buckets) over ONE weight payload: each is parsed like :func:`parse`;
    all must declare the same weights (names, shapes, dtypes, payload spans)
    and input dtype, and their input shapes must differ.  The server builds
    one graph per shape on shared weight tensors and routes each request by
    its input shape."""
    _req(isinstance(objs, list) and 1 <= len(objs) <= MAX_VARIANTS,
         f"a tenant registers 1 to {MAX_VARIANTS} program variants")
    progs = [parse(o, payload, gpu=gpu) for o in objs]
    p0 = progs[0]
    seen = set()
    for p in progs:
        sig = {k: (v.shape, v.dtype) for k, v in p.params.items()}
        _req(sig == {k: (v.shape, v.dtype) for k, v in p0.params.items()} and p.param_layout == p0.param_layout,
             f"variant {p.name!r} declares other weights than {p0.name!r}: variants share one weight payload")
        _req(p.inputs[0].dtype == p0.inputs[0].dtype, "variants take the same input dtype")
        _req({k: (v.shape, v.dtype) for k, v in p.state.items()} == {k: (v.shape, v.dtype) for k, v in p0.state.items()},
             f"variant {p.name!r} declares other state than {p0.name!r}: variants share one state")
        _req(p.inputs[0].shape not in seen, f"two variants take the input shape {list(p.inputs[0].shape)}")
        seen.add(p.inputs[0].shape)
    _req(len({p.sampling_state for p in progs} - {None}) <= 1, "variants must share one sampling control state")
    _req(len({p.adapter_state for p in progs} - {None}) <= 1, "variants must share one adapter state")
    for what in ("stopping_state", "done_state", "seen_state", "speculate_state", "hist_state"):
        _req(len({getattr(p, what) for p in progs} - {None}) <= 1,
             f"variants must share one {what.replace('_', ' ')} (the stopping control words, the done flags, the "
             f"bitmap; the speculation control words, the token history)")
    return progs


def parse(obj: dict, payload: bytes | memoryview = b"", gpu: bool = False) -> Program:
    """Validate a wire program (see the module docstring) against its payload;
    ``gpu``: also check the native kernels' shape constraints."""
    _req(isinstance(obj, dict), "program must be a JSON object")
    _req(obj.get("format") == FORMAT, f"program format must be {FORMAT!r}")
    extra = set(obj) - {"format", "name", "inputs", "params", "state", "nodes", "outputs", "meta"}
    _req(not extra, f"unknown program keys {sorted(extra)}")
    name = str(obj.get("name", "program"))[:128]
    values: dict[str, Value] = {}

    def define(v: Value) -> None:
        _req(v.name not in values, f"value {v.name!r} is defined twice")
        values[v.name] = v

    ins = obj.get("inputs")
    _req(isinstance(ins, list) and len(ins) == 1, "a program takes exactly one input")
    inputs = []
    for d in ins:
        _req(isinstance(d, dict), "inputs must be objects")
        dt = d.get("dtype", "fp32")
        _req(dt != "u8", "input dtype u8 is the MXFP4 codes' and block scales': a u8 value is a param, read only as "
             "input 1 or 2 of linear_mx4")
        _req(dt in WIRE_DTYPES and dt != "i8", f"input dtype must be one of {sorted(set(WIRE_DTYPES) - {'i8', 'u8'})}")
        v = Value(_name(d.get("name"), "input name"), _shape(d.get("shape"), "input shape"), dt, "input")
        define(v)
        inputs.append(v)
    ps = obj.get("params", [])
    _req(isinstance(ps, list) and len(ps) <= MAX_PARAMS, f"params must be a list of at most {MAX_PARAMS}")
    params: dict[str, Value] = {}
    layout: dict[str, tuple[int, int]] = {}
    spans = []
    for d in ps:
        _req(isinstance(d, dict), "params must be objects")
        dt = d.get("dtype", "fp32")
        _req(dt in PARAM_DTYPES, f"param dtype must be one of {PARAM_DTYPES}")
        v = Value(_name(d.get("name"), "param name"), _shape(d.get("shape"), "param shape"), dt, "param")
        off, nb = _int(d.get("offset"), "param offset", 0), _int(d.get("nbytes"), "param nbytes", 0)
        _req(nb == v.nbytes, f"param {v.name!r}: nbytes {nb} != {v.nbytes} for {v.shape} {dt}")
        _req(off % WIRE_DTYPES[dt] == 0, f"param {v.name!r}: offset must be {dt}-aligned")
        _req(off + nb <= len(payload), f"param {v.name!r} lies outside the {len(payload)}-byte payload")
        define(v)
        params[v.name] = v
        layout[v.name] = (off, nb)
        spans.append((off, off + nb, v.name))
    spans.sort()
    for (a0, a1, an), (b0, _b1, bn) in zip(spans, spans[1:]):
        _req(b0 >= a1, f"params {an!r} and {bn!r} overlap in the payload")
    st = obj.get("state", [])
    _req(isinstance(st, list) and len(st) <= MAX_STATE, f"state must be a list of at most {MAX_STATE}")
    state: dict[str, Value] = {}
    for d in st:
        _req(isinstance(d, dict) and set(d) <= {"name", "shape", "dtype"}, "a state is {name, shape, dtype}")
        dt = d.get("dtype", "fp32")
        _req(dt != "u8", "state dtype u8 is the MXFP4 codes' and block scales': a u8 value is a param, read only as "
             "input 1 or 2 of linear_mx4")
        _req(dt in STATE_DTYPES, f"state dtype must be one of {STATE_DTYPES}")
        v = Value(_name(d.get("name"), "state name"), _shape(d.get("shape"), "state shape"), dt, "state")
        define(v)
        state[v.name] = v
    # state versions: root name -> its current version; an in-place writer's
    # output becomes the current version and the one it consumed is dead
    current = {k: k for k in state}
    root_of = {k: k for k in state}
    dead: set[str] = set()
    sampling = None   # the control state of the program's sample nodes
    # a stopping program's control words, flags and bitmap; a speculating program's history and control words
    stop = {"stopping": None, "done": None, "seen": None, "hist": None, "speculate": None}
    adapter = None    # the state the program's lora nodes read as sel (one per program)
    cache_rows: dict[int, str] = {}     # the lengths L of the caches [B, L, Hkv, D] the kv_writes fill -> a node
    spec_limits: dict[int, str] = {}    # the ``limit`` of every spec_accept -> a node
    scales_of: dict[str, str] = {}      # a scales state -> the i8 cache (root) whose row scales it holds
    cache_scales: dict[str, str] = {}   # and back
    other_use: dict[str, str] = {}      # a state -> the first node naming it as anything but a cache's scales
    rings: dict[str, tuple] = {}        # a cache (root) -> the (window, limit) every node naming it carries, or None
    ns = obj.get("nodes")
    _req(isinstance(ns, list) and 0 < len(ns) <= MAX_NODES, f"nodes must be a list of 1..{MAX_NODES}")
    nodes = []
    for d in ns:
        _req(isinstance(d, dict) and set(d) <= {"op", "inputs", "output", "attrs"}, "a node is {op, inputs, output, attrs}")
        op = d.get("op")
        _req(op in OPS, f"op {op!r} is not one the pod server runs (whitelist: {' '.join(OPS)})")
        refs = d.get("inputs")
        _req(isinstance(refs, list) and refs, f"node of op {op}: inputs must be a non-empty list")
        for r in refs:
            _req(isinstance(r, str) and r in values, f"node of op {op}: input {r!r} is not defined before it")
            _req(r not in dead, f"node of op {op}: state version {r!r} was updated in place before this node "
                 f"(use {current.get(root_of.get(r, r), r)!r})")
        attrs = d.get("attrs") or {}
        _req(isinstance(attrs, dict), "attrs must be an object")
        n = Node(op, list(refs), _name(d.get("output"), "node output"), dict(attrs))
        # an i8 value is a quantized weight (only linear_q8 reads it, as its weight) or a quantized
        # cache state (only kv_write / sdpa_cache take it, as their cache)
        slots = _Q8_CACHE_SLOTS.get(op, {})
        for k, r in enumerate(refs):
            if values[r].dtype != "i8":
                continue
            if r in root_of:
                _req(k in slots, f"node {n.output!r} ({op}): input {r!r} is an i8 state; only kv_write and "
                     f"sdpa_cache take one, as their cache")
            else:
                _req((op == "linear_q8" and k == 1) or (op == "moe_q8" and k in (2, 4)), f"node {n.output!r} ({op}): input {r!r} is an i8 param; only "
                     f"linear_q8 takes one, as its weight")
        # a u8 value is an MXFP4 weight's codes or block scales: only linear_mx4 reads it, as input 1 or 2
        for k, r in enumerate(refs):
            _req(values[r].dtype != "u8" or (op == "linear_mx4" and k in (1, 2)) or (op == "moe_mx4" and 2 <= k <= 5),
                 f"node {n.output!r} ({op}): input {k} {r!r} is a u8 param; only linear_mx4 takes one, as its codes "
                 f"(input 1) or its block scales (input 2)")
        shape, dt = _infer(n, [values[r] for r in refs], gpu)
        _req(math.prod(shape) <= MAX_NUMEL, f"node {n.output!r}: output too large")
        # a scales state is not versioned: it is named only beside versions of its ONE cache, so the
        # cache's version chain orders its reads and writes too
        as_scales = set()
        for ck, sk in slots.items():
            if values[refs[ck]].dtype != "i8":
                continue
            root, sname = root_of[refs[ck]], refs[sk]
            _req(scales_of.setdefault(sname, root) == root,
                 f"node {n.output!r} ({op}): scales state {sname!r} belongs to the cache {scales_of[sname]!r}; "
                 f"it cannot also hold the scales of {root!r}")
            _req(cache_scales.setdefault(root, sname) == sname,
                 f"node {n.output!r} ({op}): the cache {root!r} keeps its scales in {cache_scales[root]!r}, "
                 f"not in {sname!r}")
            as_scales.add(sk)
        for k, r in enumerate(refs):
            if r in state and k not in as_scales:
                other_use.setdefault(r, f"node {n.output!r} ({op})")
        if op in STATE_WRITERS:
            tgt = refs[0]
            _req(tgt in root_of, f"node {n.output!r} ({op}): updates a state in place; {tgt!r} is not one")
            _req(refs.count(tgt) == 1, f"node {n.output!r} ({op}): the updated state cannot also be an operand")
            dead.add(tgt)
            root_of[n.output] = root_of[tgt]
            current[root_of[tgt]] = n.output
        if op == "sample":
            _req(sampling in (None, refs[1]), f"node {n.output!r} (sample): a program has one control state; "
                 f"{sampling!r} and {refs[1]!r} are two")
            sampling = refs[1]
        for role, k in _STOP_ROLES.get(op, ()):
            if k >= len(refs):   # pos_add's optional mask
                continue
            r = refs[k]
            root = root_of.get(r, r)
            _req(root in state, f"node {n.output!r} ({op}): {role} must be a state (or a version of one); {r!r} is not")
            _req(stop[role] in (None, root), f"node {n.output!r} ({op}): a program has one {role} state; "
                 f"{stop[role]!r} and {root!r} are two")
            stop[role] = root
        if op == "lora":
            _req(adapter in (None, refs[3]), f"node {n.output!r} (lora): a program has one adapter state; "
                 f"{adapter!r} and {refs[3]!r} are two")
            adapter = refs[3]
        for ck in {"kv_write": (0,), "sdpa_cache": (1, 2)}.get(op, ()):
            root = root_of.get(refs[ck])
            _req(root is not None or "window" not in attrs, f"node {n.output!r} ({op}): a ring cache must be a state "
                 f"(or a version of one); {refs[ck]!r} is not")
            ring = (attrs["window"], attrs["limit"]) if "window" in attrs else None
            if root is not None:
                _req(rings.setdefault(root, ring) == ring, f"node {n.output!r} ({op}): the cache {root!r} is "
                     f"{_ring_name(rings[root])} in an earlier node and {_ring_name(ring)} here")
        if op == "kv_write":   # the positions the write keeps: a ring's limit, else the cache's rows
            cache_rows.setdefault(attrs.get("limit", values[refs[0]].shape[1]), f"node {n.output!r} ({op})")
        if op == "spec_accept":
            spec_limits.setdefault(attrs["limit"], f"node {n.output!r} ({op})")
        define(Value(n.output, shape, dt, "node"))
        nodes.append(n)
    outs = obj.get("outputs")
    _req(isinstance(outs, list) and outs and all(isinstance(o, str) and o in values for o in outs),
         "outputs must name defined values")
    for k, v in state.items():
        _req(v.dtype != "i8" or k in cache_scales, f"state {k!r}: state dtype i8 is a quantized K / V cache's; "
             f"no kv_write / sdpa_cache node names it as its cache")
    for s_ in scales_of:
        _req(s_ not in other_use, f"{other_use.get(s_)}: {s_!r} holds the scales of the i8 cache {scales_of[s_]!r}; "
             f"a scales state is named only beside that cache in kv_write / sdpa_cache")
        _req(s_ not in outs, f"the scales state {s_!r} of the i8 cache {scales_of[s_]!r} cannot be an output")
    # the control states: at most one of each kind, and each its own state
    ctls = [c for c in (sampling, stop["stopping"], stop["speculate"], adapter) if c is not None]
    _req(len(set(ctls)) == len(ctls), f"the control states of different kinds must be different states, got {ctls}")
    if stop["hist"] is not None:   # positions index the history as they index the caches
        L = state[stop["hist"]].shape[1]
        for rows, where in {**cache_rows, **spec_limits}.items():
            _req(rows == L, f"{where}: the token history {stop['hist']!r} has {L} positions, the "
                 f"{'caches have' if rows in cache_rows else 'limit is'} {rows}: hist must be [batch, L] with L the caches' length")
    else:
        _req(not spec_limits, "a spec_accept needs the program's token history (a hist_write or spec_draft node)")
    _req(adapter not in outs, f"the adapter state {adapter!r} cannot be an output: it is a control state")
    _req(not any(o in root_of for o in outs), "a state (or a version of one) cannot be an output: it is mutable")
    _req(not any(values[o].dtype == "i8" for o in outs), "an i8 param cannot be an output")
    _req(not any(values[o].dtype == "u8" for o in outs), "a u8 param cannot be an output: MXFP4 codes and block scales "
         "are read only by linear_mx4")
    return Program(name, inputs, params, layout, nodes, list(outs), values, payload, state=state,
                   state_root={k: v for k, v in root_of.items() if k != v}, sampling_state=sampling,
                   stopping_state=stop["stopping"], done_state=stop["done"], seen_state=stop["seen"],
                   speculate_state=stop["speculate"], hist_state=stop["hist"], adapter_state=adapter)

