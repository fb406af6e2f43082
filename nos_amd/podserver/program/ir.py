"""Program IR: values, nodes, limits and the op sets (shared by the
validator, the accounting, the compiler and the executor)."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

FORMAT = "nos-amd.program/v1"
# i32: token ids (an input only; consumed by embedding); i8: quantized weights (a param; linear_q8's input 1)
# or a quantized K / V cache (a state; the cache operand of kv_write / sdpa_cache, with an fp32 scales state);
# u8: MXFP4 codes and E8M0 block scales (params; linear_mx4's inputs 1 and 2, nothing else)
WIRE_DTYPES = {"fp32": 4, "bf16": 2, "i32": 4, "i8": 1, "u8": 1}
PARAM_DTYPES = ("fp32", "bf16", "i8", "u8")
MX4_BLOCK = 32               # consecutive k under one scale byte (builder.quantize_rows_mx4)
MX4_SCALE_MIN, MX4_SCALE_MAX = 2, 252   # the scale bytes a registration accepts: dequantized values stay normal fp32
FLOAT_DTYPES = ("fp32", "bf16")
MAX_NODES = 8192
MAX_PARAMS = 8192
MAX_NUMEL = 1 << 31          # elements of one value
MAX_RANK = 8
MAX_VARIANTS = 8             # input shapes one tenant may register (parse_variants)
UNARY = ("gelu", "relu", "sigmoid", "silu", "tanh", "exp", "neg", "rsqrt")
BINARY = ("add", "mul", "sub", "div")
ACTS = (None, "gelu", "relu")
INTERP_MODES = ("bicubic", "bilinear", "nearest")


class ProgramError(ValueError):
    """The program is malformed or uses something the server does not run."""


@dataclass(frozen=True)
class Value:
    name: str
    shape: tuple[int, ...]
    dtype: str
    kind: str                 # "input" | "param" | "state" | "node"

    @property
    def numel(self) -> int:
        return math.prod(self.shape)

    @property
    def nbytes(self) -> int:
        return self.numel * WIRE_DTYPES[self.dtype]


@dataclass
class Node:
    op: str
    inputs: list[str]
    output: str
    attrs: dict = field(default_factory=dict)



# ---------------------------------------------------------------- validation
def _req(cond: bool, msg: str) -> None:
    if not cond:
        raise ProgramError(msg)


def _int(v, what: str, lo: int | None = None) -> int:
    _req(isinstance(v, int) and not isinstance(v, bool), f"{what} must be an integer, got {v!r}")
    if lo is not None:
        _req(v >= lo, f"{what} must be >= {lo}, got {v}")
    return v


def _dim(d, what: str) -> int:
    """One dimension: an int in [1, MAX_NUMEL] (products are then taken on
    Python ints, which cannot wrap)."""
    d = _int(d, what, 1)
    _req(d <= MAX_NUMEL, f"{what} {d} is over {MAX_NUMEL}")
    return d


def _shape(v, what: str) -> tuple[int, ...]:
    _req(isinstance(v, list) and len(v) <= MAX_RANK, f"{what} must be a list of at most {MAX_RANK} dims")
    s = tuple(_dim(d, f"{what} dim") for d in v)
    _req(math.prod(s) <= MAX_NUMEL, f"{what} has more than {MAX_NUMEL} elements")
    return s


def _name(v, what: str) -> str:
    _req(isinstance(v, str) and 0 < len(v) <= 128, f"{what} must be a non-empty string of <= 128 chars")
    return v


def _broadcast(a: tuple, b: tuple, what: str) -> tuple:
    n = max(len(a), len(b))
    a2, b2 = (1,) * (n - len(a)) + a, (1,) * (n - len(b)) + b
    out = []
    for x, y in zip(a2, b2):
        _req(x == y or x == 1 or y == 1, f"{what}: shapes {a} and {b} do not broadcast")
        out.append(max(x, y))
    return tuple(out)




def _pair(v, what: str, lo: int) -> tuple[int, int]:
    if isinstance(v, int) and not isinstance(v, bool):
        v = [v, v]
    _req(isinstance(v, list) and len(v) == 2, f"{what} must be an int or [h, w]")
    return (_int(v[0], what, lo), _int(v[1], what, lo))


def _eps(a: dict, what: str) -> None:
    eps = a.get("eps", 1e-5)
    _req(isinstance(eps, (int, float)) and not isinstance(eps, bool) and 0 < eps < 1, f"{what}: eps must be in (0, 1)")



OPS = ("linear", "layernorm", "attention", *BINARY, *UNARY, "cat", "slice", "reshape", "permute", "expand",
       "cast", "interpolate",
       # general tenants: conv nets and decoder LLMs (nos_amd/ops/tenant.py)
       "conv2d", "batchnorm", "max_pool2d", "avg_pool2d", "mean", "sum", "matmul", "softmax", "embedding",
       "rmsnorm", "rotary", "sdpa",
       # int8 weight-only linear: act(x @ (wq.float() * wscale[:, None]).T + bias), fp32 math
       "linear_q8",
       # MXFP4 weight-only linear: act(x @ dequantize_rows_mx4(wq, wscale).T + bias), fp32 math
       "linear_mx4")
# stateful decoding (round 6): ops over state buffers that persist across a
# tenant's requests (a K / V cache, a position counter).  STATE_WRITERS update
# their first input IN PLACE and return its new version (the validator makes
# the old version dead from then on, so in-place equals SSA semantics)
STATE_OPS = ("kv_write", "sdpa_cache", "rotary_at", "pos_add", "pos_set", "argmax", "sample")
STATE_WRITERS = ("kv_write", "pos_add", "pos_set")
# stop ids and repetition penalty (a stopping tenant): seen_mark(seen, ids) sets the ids' bits in
# the rows' bitmaps, penalize(logits, seen, ctl) penalises the seen tokens' logits,
# stop_ids(next, done, ctl) pads finished rows, done_mark(done, ids, ctl) finishes rows that
# drew a stop id; pos_add takes ``done`` as a second input (finished rows keep their counter)
STOP_CTL_WORDS = 8           # [penalty fp32 bits, pad_id, n_stop, stop0 .. stop3, 0] (ops.tenant.stopping_ctl)
MAX_STOP_IDS = 4
STOP_OPS = ("seen_mark", "penalize", "stop_ids", "done_mark")
STATE_OPS = STATE_OPS + STOP_OPS
STATE_WRITERS = STATE_WRITERS + ("seen_mark", "done_mark")
# speculative decoding (a speculating tenant): hist_write(hist, pos, ids[, tail[, n]]) keeps the
# rows' token history, spec_accept(ids, g, pos, ctl) is a verify step's advance per row,
# pos_advance(pos, n) adds it to the counters, spec_draft(hist, pos) looks the next drafts up
SPEC_CTL_WORDS = 4           # [end, 0, 0, 0] (ops.tenant.speculate_ctl)
SPEC_MIN_K, SPEC_MAX_K = 2, 8
SPEC_OPS = ("hist_write", "spec_accept", "pos_advance", "spec_draft")
STATE_OPS = STATE_OPS + SPEC_OPS
STATE_WRITERS = STATE_WRITERS + ("hist_write", "pos_advance")
# multi-adapter LoRA (an adapter tenant): lora(x, A, B, sel) is the low-rank delta of the adapter each
# sequence's ``sel`` names (0: none), added to a linear's output; ``sel`` is the program's adapter state
LORA_MAX_RANK = 64           # the stacked rank R of one lora node (the GEMV epilogue stages t [rows, R] in LDS)
STATE_OPS = STATE_OPS + ("lora",)
STATE_DTYPES = ("fp32", "bf16", "i32", "i8")
MAX_STATE = 1024
# mixture of experts (a Mixtral-class tenant): moe(x, Wr, W13, W2; top_k) is a sparse MoE MLP whose expert
# weights are chosen per row by a value computed on the device (ops.tenant.moe_ref)
MOE_MAX_EXPERTS = 64         # a lane per expert in the route kernel
MOE_MAX_TOP_K = 8
# quantized experts: moe_q8(x, Wr, W13q, s13, W2q, s2; top_k) holds the expert tensors as int8 rows with an fp32
# scale per row, moe_mx4(x, Wr, W13c, W13e, W2c, W2e; top_k) as MXFP4 codes and E8M0 block scales (storage
# formats: moe over the dequantized experts, ops.tenant.moe_q8_ref / moe_mx4_ref); the router stays fp32
MOE_OPS = ("moe", "moe_q8", "moe_mx4")
OPS = OPS + STATE_OPS + MOE_OPS
# linear_q8: folding it would materialise the fp32 weight the format exists to avoid
NEVER_FOLD = ("attention", "sdpa", "linear_q8", "linear_mx4", *MOE_OPS, *STATE_OPS)
QUANT_LINEARS = ("linear_q8", "linear_mx4")   # weight-only linears: (x, wq, wscale, [bias]), never folded
# step kinds that run a gfx950 kernel of libnos_hip.so (CompiledProgram.stats["kernels"])
NATIVE_KINDS = ("linear", "linear_ln", "linear_rms", "ln_qkv_attention", "attention", "layernorm", "conv2d", "matmul",
                "softmax", "embedding", "rmsnorm", "rotary", "sdpa", "patches", "unary", "kv_write", "sdpa_cache",
                "rotary_at", "pos_add", "pos_set", "argmax", "sample", "glu", "linear_q8", "linear_mx4", *STOP_OPS, "stop_step", *SPEC_OPS, "spec_step", "lora_shrink",
                "moe_route", "moe_glu", "moe_down", "moe_glu_q8", "moe_down_q8", "moe_glu_mx4", "moe_down_mx4")
# the steps a speculating tenant's verify program closes with (CompiledProgram.stats["spec_launches"]);
# spec_step: spec_accept / hist_write / pos_advance / spec_draft fused into one launch
SPEC_KINDS = (*SPEC_OPS, "spec_step")
# the steps a stopping program adds to a plain one (CompiledProgram.stats["stop_launches"]); stop_step:
# the pos_add(pos, done) / stop_ids / done_mark trio fused into one launch
STOP_KINDS = (*STOP_OPS, "stop_step")
GEMM_OPS = ("linear", "conv2d")


def torch_dtype(dt: str):
    import torch

    return {"fp32": torch.float32, "bf16": torch.bfloat16, "i32": torch.int32, "i8": torch.int8,
            "u8": torch.uint8}[dt]
