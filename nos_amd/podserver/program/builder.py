"""Building wire programs with numpy only (the pod side never imports
torch), saving / loading them, and the GEMM-MLP probe tenant."""
from __future__ import annotations

import math

import numpy as np

from .ir import FORMAT


def bf16_bits(a: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns (round to nearest even), as uint16."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + 0x7FFF
    return ((u + r) >> 16).astype(np.uint16)


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def quantize_rows_q8(w: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Symmetric int8 quantization of a weight [N, K], one scale per output row:
    ``scale = max|row| / 127`` (1.0 for an all-zero row) and
    ``q = clip(rint(row / scale), -127, 127)``.  Returns (q int8 [N, K], scale
    fp32 [N]); :func:`dequantize_rows_q8` gives the weight the server computes with."""
    a = np.ascontiguousarray(w, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError(f"quantize_rows_q8 takes a [N, K] weight, got {a.shape}")
    amax = np.abs(a).max(axis=1) if a.shape[1] else np.zeros(a.shape[0], np.float32)
    scale = np.where(amax > 0, amax / np.float32(127), np.float32(1)).astype(np.float32)
    q = np.clip(np.rint(a / scale[:, None]), -127, 127).astype(np.int8)
    return q, scale


def dequantize_rows_q8(q: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """``q.astype(fp32) * scale[:, None]`` in fp32 (one rounding per element): the
    weight a ``linear_q8`` node means."""
    return np.asarray(q).astype(np.float32) * np.asarray(scale, dtype=np.float32)[:, None]


MX4_BLOCK = 32                   # consecutive k of a row that share one E8M0 scale byte
MX4_SCALE_MIN, MX4_SCALE_MAX = 2, 252   # the scale bytes in use: every dequantized value is a normal, finite fp32
# the E2M1 element of each 4-bit code: bit 3 the sign, bits 2..0 the magnitude
MX4_VALUES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], np.float32)


def quantize_rows_mx4(w: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """OCP Microscaling MXFP4 of a weight [N, K], K % 32 == 0: 4-bit E2M1 elements, each block of 32
    consecutive k of a row under one E8M0 power-of-two scale.  The scale byte of a block is ``e =
    clamp(floor(log2(max|v|)) - 2 + 127, 2, 252)`` (the exponent taken exactly, from ``frexp``; 127 for
    an all-zero block; 255, the format's NaN, never).  ``v / 2^(e - 127)`` is rounded to the nearest of
    +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even code, saturating at +-6; the sign is the code's
    bit 3.  Element 2 i sits in the low nibble of byte i, element 2 i + 1 in the high one.  Returns
    (codes u8 [N, K / 2], scales u8 [N, K / 32]); :func:`dequantize_rows_mx4` gives the weight the
    server computes with."""
    a = np.ascontiguousarray(w, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] % MX4_BLOCK:
        raise ValueError(f"quantize_rows_mx4 takes a [N, K] weight with K % {MX4_BLOCK} == 0 (a scale byte per "
                         f"{MX4_BLOCK} consecutive k), got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError("quantize_rows_mx4 takes finite weights")
    N, K = a.shape
    blk = a.reshape(N, K // MX4_BLOCK, MX4_BLOCK)
    amax = np.abs(blk).max(axis=2) if K else np.zeros((N, 0), np.float32)
    _, ex = np.frexp(amax)                       # amax = m 2^ex with 0.5 <= m < 1: floor(log2) = ex - 1
    e = np.where(amax > 0, np.clip(ex.astype(np.int64) - 3 + 127, MX4_SCALE_MIN, MX4_SCALE_MAX), 127)
    mag = np.abs(np.ldexp(blk.astype(np.float64), (127 - e)[:, :, None]))   # exact in fp64
    # the midpoints between neighbouring magnitudes; a tie goes to the even code of the two
    code = ((mag > 0.25).astype(np.uint8) + (mag >= 0.75) + (mag > 1.25) + (mag >= 1.75) + (mag > 2.5)
            + (mag >= 3.5) + (mag > 5.0)).astype(np.uint8)
    code |= (np.signbit(blk).astype(np.uint8) << 3)
    code = code.reshape(N, K)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8), e.astype(np.uint8)


def dequantize_rows_mx4(codes: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """``elem * 2^(e - 127)`` as fp32 [N, K] (exact: a power-of-two scale of a 2-bit significand): the
    weight a ``linear_mx4`` node means."""
    c = np.asarray(codes, dtype=np.uint8)
    s = np.asarray(scales, dtype=np.uint8)
    if c.ndim != 2 or s.ndim != 2 or c.shape[0] != s.shape[0] or c.shape[1] * 2 != s.shape[1] * MX4_BLOCK:
        raise ValueError(f"dequantize_rows_mx4 takes codes [N, K / 2] and scales [N, K / {MX4_BLOCK}], got {c.shape} "
                         f"and {s.shape}")
    el = np.empty((c.shape[0], c.shape[1] * 2), np.float32)
    el[:, 0::2] = MX4_VALUES[c & 15]
    el[:, 1::2] = MX4_VALUES[c >> 4]
    return np.ldexp(el, np.repeat(s.astype(np.int32) - 127, MX4_BLOCK, axis=1)).astype(np.float32)


def _rows_of_experts(quantize, w: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """``quantize`` (a rows quantizer of [N, K]) on a 2-D weight as it is, on a 3-D [E, N, K] on the rows
    flattened to [E * N, K] with both outputs shaped back to [E, N, ...]."""
    a = np.asarray(w)
    if a.ndim != 3:
        return quantize(w)
    E, N, K = a.shape
    q, s = quantize(a.reshape(E * N, K))
    return q.reshape(E, N, *q.shape[1:]), s.reshape(E, N, *s.shape[1:])


class Builder:
    """Assemble a wire program with numpy only (the pod side never imports
    torch).  ``param`` appends a weight to the payload; op methods append
    nodes and return the output's name."""

    def __init__(self, name: str):
        self.name = name
        self.inputs: list[dict] = []
        self.params: list[dict] = []
        self.nodes: list[dict] = []
        self.states: list[dict] = []
        self.chunks: list[bytes] = []
        self.offset = 0
        self._n = 0

    def input(self, name: str, shape, dtype: str = "fp32") -> str:
        self.inputs.append({"name": name, "shape": list(shape), "dtype": dtype})
        return name

    def param(self, name: str, array: np.ndarray, dtype: str = "fp32") -> str:
        a = np.ascontiguousarray(array, dtype=np.float32)
        raw = (a if dtype == "fp32" else bf16_bits(a)).tobytes()
        self.params.append({"name": name, "shape": list(a.shape), "dtype": dtype, "offset": self.offset,
                            "nbytes": len(raw)})
        self.chunks.append(raw)
        self.offset += len(raw)
        return name

    def param_q8(self, name: str, w_fp32: np.ndarray) -> tuple[str, str]:
        """An fp32 weight [N, K] stored as int8 rows + fp32 row scales
        (:func:`quantize_rows_q8`): the params ``name + ".q8"`` (i8) and
        ``name + ".scale"`` a ``linear_q8`` node takes.  A 3-D weight [E, N, K] (an expert tensor of a
        ``moe_q8`` node) is quantized by the same rule on its rows flattened to [E * N, K]: q8 [E, N, K] and
        scale [E, N]."""
        q, scale = _rows_of_experts(quantize_rows_q8, w_fp32)
        raw = q.tobytes()
        self.params.append({"name": name + ".q8", "shape": list(q.shape), "dtype": "i8", "offset": self.offset,
                            "nbytes": len(raw)})
        self.chunks.append(raw)
        self.offset += len(raw)
        pad = -self.offset % 4   # the fp32 params after it stay 4-byte aligned in the payload
        if pad:
            self.chunks.append(b"\0" * pad)
            self.offset += pad
        return name + ".q8", self.param(name + ".scale", scale)

    def _param_u8(self, name: str, a: np.ndarray) -> str:
        raw = a.tobytes()
        self.params.append({"name": name, "shape": list(a.shape), "dtype": "u8", "offset": self.offset,
                            "nbytes": len(raw)})
        self.chunks.append(raw)
        self.offset += len(raw)
        pad = -self.offset % 4   # the params after it stay 4-byte aligned in the payload
        if pad:
            self.chunks.append(b"\0" * pad)
            self.offset += pad
        return name

    def param_mx4(self, name: str, w_fp32: np.ndarray) -> tuple[str, str]:
        """An fp32 weight [N, K] stored as MXFP4 (:func:`quantize_rows_mx4`): the u8 params
        ``name + ".mx4"`` (codes [N, K / 2]) and ``name + ".e8m0"`` (block scales [N, K / 32]) a
        ``linear_mx4`` node takes.  A 3-D weight [E, N, K] (an expert tensor of a ``moe_mx4`` node) is
        quantized by the same rule on its rows flattened to [E * N, K]: mx4 [E, N, K / 2] and e8m0 [E, N, K / 32]."""
        codes, scales = _rows_of_experts(quantize_rows_mx4, w_fp32)
        return self._param_u8(name + ".mx4", codes), self._param_u8(name + ".e8m0", scales)

    def state(self, name: str, shape, dtype: str = "fp32") -> str:
        """A state buffer (zero at registration, kept across requests)."""
        self.states.append({"name": name, "shape": list(shape), "dtype": dtype})
        return name

    def cache_q8(self, name: str, scales: str, shape) -> tuple[str, str]:
        """A K / V cache [B, L, Hkv, D] kept as int8 rows with one fp32 scale per row: the i8
        state ``name`` and its fp32 [B, L, Hkv] state ``scales`` (``kv_write`` takes the scales as
        input 3, ``sdpa_cache`` K's and V's as inputs 4 and 5; the server quantizes the rows as it
        writes them, by :func:`quantize_rows_q8`'s rule)."""
        return self.state(name, shape, "i8"), self.state(scales, list(shape)[:3], "fp32")

    def stopping_states(self, batch: int, vocab: int, done: str = "done", seen: str = "seen",
                        ctl: str = "stopping") -> tuple[str, str, str]:
        """The three states of a stopping program (stop ids, repetition penalty): the rows' ``done``
        flags i32 [batch], the ``seen`` bitmaps i32 [batch, ceil(vocab / 32)] (bit ``id & 31`` of word
        ``id >> 5``: token ``id`` is in the row's sequence) and the control words ``ctl`` i32 [8] the
        server fills from each request's ``"stopping"`` field (``ops.tenant.stopping_ctl``)."""
        return (self.state(done, [batch], "i32"), self.state(seen, [batch, -(-vocab // 32)], "i32"),
                self.state(ctl, [8], "i32"))

    def speculate_states(self, batch: int, max_len: int, hist: str = "hist",
                         ctl: str = "speculate") -> tuple[str, str]:
        """The two states of a speculating program: the rows' token history ``hist`` i32 [batch,
        max_len] (``hist[b, t]``: the token at position t, for every t up to and including the
        pending one at ``pos[b]``) and the control words ``ctl`` i32 [4] the server fills from each
        request's ``"speculate"`` field (``ops.tenant.speculate_ctl``)."""
        return self.state(hist, [batch, max_len], "i32"), self.state(ctl, [4], "i32")

    def adapter_state(self, batch: int, name: str = "adapter") -> str:
        """The control state of an adapter program: i32 [batch], the LoRA adapter of each sequence
        (1 .. n; 0 or anything out of range: the base model), which the server fills from each
        request's ``"adapter"`` field and every ``lora`` node reads as its ``sel``."""
        return self.state(name, [batch], "i32")

    def moe(self, x: str, router: str, gate_up: str, down: str, top_k: int, out: str | None = None) -> str:
        """A sparse mixture-of-experts MLP over x [..., H]: ``router`` [E, H], ``gate_up`` [E, 2I, H] (gate rows,
        then up rows) and ``down`` [E, H, I] are fp32 params; each row takes its ``top_k`` experts
        (``ops.tenant.moe_ref``)."""
        return self.op("moe", x, router, gate_up, down, out=out, top_k=int(top_k))

    def moe_q8(self, x: str, router: str, gate_up_q8: str, gate_up_scale: str, down_q8: str, down_scale: str,
               top_k: int, out: str | None = None) -> str:
        """:meth:`moe` over int8 experts: ``gate_up_q8`` [E, 2I, H] / ``down_q8`` [E, H, I] i8 and their fp32 row
        scales [E, 2I] / [E, H] (:meth:`param_q8` of the 3-D tensors); the router stays fp32
        (``ops.tenant.moe_q8_ref``)."""
        return self.op("moe_q8", x, router, gate_up_q8, gate_up_scale, down_q8, down_scale, out=out, top_k=int(top_k))

    def moe_mx4(self, x: str, router: str, gate_up_mx4: str, gate_up_e8m0: str, down_mx4: str, down_e8m0: str,
                top_k: int, out: str | None = None) -> str:
        """:meth:`moe` over MXFP4 experts: codes ``gate_up_mx4`` [E, 2I, H / 2] / ``down_mx4`` [E, H, I / 2] u8 and
        their block scales [E, 2I, H / 32] / [E, H, I / 32] u8 (:meth:`param_mx4` of the 3-D tensors); the router
        stays fp32 (``ops.tenant.moe_mx4_ref``)."""
        return self.op("moe_mx4", x, router, gate_up_mx4, gate_up_e8m0, down_mx4, down_e8m0, out=out, top_k=int(top_k))

    def op(self, op: str, *inputs: str, out: str | None = None, **attrs) -> str:
        self._n += 1
        out = out or f"%{self._n}"
        self.nodes.append({"op": op, "inputs": list(inputs), "output": out,
                           "attrs": {k: v for k, v in attrs.items() if v is not None}})
        return out

    def build(self, outputs: list[str]) -> tuple[dict, bytes]:
        prog = {"format": FORMAT, "name": self.name, "inputs": self.inputs, "params": self.params,
                "nodes": self.nodes, "outputs": list(outputs)}
        if self.states:
            prog["state"] = self.states
        return prog, b"".join(self.chunks)


def save_program(prefix: str, program: dict, weights: bytes) -> None:
    """A built program as ``<prefix>.json`` + ``<prefix>.bin`` (a tenant
    builds once -- e.g. with torch.fx -- and its pods ship the files)."""
    import json

    with open(prefix + ".json", "w") as f:
        json.dump(program, f)
    with open(prefix + ".bin", "wb") as f:
        f.write(weights)


def load_program(prefix: str) -> tuple[dict, bytes]:
    """:func:`save_program`'s files back (JSON + raw bytes: nothing executable)."""
    import json

    with open(prefix + ".json") as f:
        program = json.load(f)
    with open(prefix + ".bin", "rb") as f:
        return program, f.read()


def mlp_program(dim: int = 1024, layers: int = 4, batch: int = 256, dtype: str = "bf16", seed: int = 0,
                hidden: int | None = None) -> tuple[dict, bytes]:
    """The GEMM-MLP probe tenant (BASELINE config 4's workload): ``layers``
    pre-LN residual MLP blocks (LN -> fc1 + GELU -> fc2 + residual) on a
    ``batch x dim`` activation; every block lowers onto two GEMMs with fused
    LN prologue / GELU and residual epilogues."""
    rng = np.random.default_rng(seed)
    hid = hidden or 4 * dim
    b = Builder(f"mlp-{dim}x{layers}")
    x = b.input("x", [batch, dim], "fp32")
    h = b.op("cast", x, dtype=dtype) if dtype != "fp32" else x
    for i in range(layers):
        g = b.param(f"l{i}.ln_w", 1.0 + 0.1 * rng.standard_normal(dim), dtype)
        be = b.param(f"l{i}.ln_b", 0.1 * rng.standard_normal(dim), dtype)
        w1 = b.param(f"l{i}.fc1_w", rng.standard_normal((hid, dim)) / math.sqrt(dim), dtype)
        b1 = b.param(f"l{i}.fc1_b", 0.02 * rng.standard_normal(hid), dtype)
        w2 = b.param(f"l{i}.fc2_w", rng.standard_normal((dim, hid)) / math.sqrt(hid), dtype)
        b2 = b.param(f"l{i}.fc2_b", 0.02 * rng.standard_normal(dim), dtype)
        y = b.op("layernorm", h, g, be, eps=1e-5)
        y = b.op("gelu", b.op("linear", y, w1, b1))
        h = b.op("add", b.op("linear", y, w2, b2), h)
    return b.build([h])

