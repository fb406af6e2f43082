"""A validated program (:class:`Program`): its device-memory accounting
(the static estimate the server checks against the slice before a build),
its weights as tensors, and the entry points to the compiler and the eager
reference."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .ir import GEMM_OPS, MOE_OPS, MX4_SCALE_MAX, MX4_SCALE_MIN, NEVER_FOLD, QUANT_LINEARS, Node, Value, torch_dtype
from .reference import _eager

def _workspace(node: Node, ins: list[Value], out: Value, f32_math: str) -> int:
    """Transient device bytes one op allocates while it runs, beyond its
    inputs and output (an upper bound; :meth:`Program.bytes_estimate_for`)."""
    op = node.op
    if op == "linear" and ins[0].dtype == "fp32" and f32_math == "h3":
        m = ins[0].numel // ins[0].shape[-1]
        return ins[0].nbytes + 4 * m                       # A's fp16 planes + row scales
    if op == "linear_rms" or (op == "linear" and ins[0].dtype == "bf16" and f32_math == "h3"):
        m = ins[0].numel // ins[0].shape[-1]
        return 2 * m * ins[0].shape[-1] * 4 + 4 * m + out.numel * 4
    if op == "attention":
        b, s, three_hd = ins[0].shape
        h = node.attrs["heads"]
        return _attn_ws(b, s, s, h, h, three_hd // (3 * h)) + ins[0].nbytes + out.numel * 4
    if op == "sdpa":
        (b, sq, h, d), (_, skv, hkv, _) = ins[0].shape, ins[1].shape
        copies = sum(v.numel * 4 for v in ins[:3]) if ins[0].dtype != "fp32" else 0
        return _attn_ws(b, sq, skv, h, hkv, d) + copies + out.numel * 4
    if op == "conv2d":
        n, c, _, _ = ins[0].shape
        oc, cg, kh, kw = ins[1].shape
        p = out.numel // (n * oc)
        kp = -(-(cg * kh * kw) // 32) * 32
        return n * (c // cg) * p * (kp * 4 + 4) + ins[0].numel * 4 + out.numel * 4
    if op in QUANT_LINEARS:
        # decode rows run on the int8 / MXFP4 GEMV; more dequantize the weight into a transient fp32
        # buffer for the run-time-split h3 product (ops.tenant.linear_q8, linear_mx4)
        k = ins[0].shape[-1]
        m, n = ins[0].numel // k, ins[1].shape[0]
        if m <= 8:
            return 0
        kp = -(-k // 32) * 32
        return n * k * 4 + (m + n) * kp * 12 + out.numel * 4
    if op == "lora":
        # decode rows: t [rows, R] between the shrink launch and the GEMV that expands it; more rows
        # (a prefill) gather each sequence's A and B and hold t and the masked delta beside the output
        b, s, k = ins[0].shape
        r, n = ins[1].shape[1], ins[2].shape[1]
        if b * s <= 8:
            return b * s * r * 4
        return b * (r * k + n * r) * 4 + b * s * r * 4 + 2 * out.numel * 4
    if op in MOE_OPS:
        # decode rows: idx and w [rows, k] and act [rows, k, I] between the three launches; more rows (a
        # prefill) run dense over the experts: the gates [rows, E] and, per expert, the merged product
        # [rows, 2I], its activation [rows, I] and the down product and running sum [rows, H] (the expert
        # weights themselves are params: charged once, never copied)
        # quantized experts (moe_q8, moe_mx4): decode rows as moe; a prefill also holds ONE expert's two tensors
        # dequantized into fp32 at a time ((2I H + H I) x 4 bytes), never all of them
        h = ins[0].shape[-1]
        rows, (e, i2, _), k = ins[0].numel // h, ins[2].shape, node.attrs["top_k"]
        if rows <= 8:
            return rows * k * (8 + i2 // 2 * 4)
        one = (i2 * h + h * (i2 // 2)) * 4 if op != "moe" else 0
        return rows * (3 * e + 2 * k) * 4 + rows * (i2 + i2 // 2 + 3 * h) * 4 + one
    if op == "matmul":
        k = ins[0].shape[-1]
        kp = -(-k // 32) * 32
        rows = ins[0].numel // k + ins[1].numel // k
        return rows * kp * 12 + out.numel * 4          # padded fp32 copies + planes + the fp32 result
    return 0


def _attn_ws(b: int, sq: int, skv: int, h: int, hkv: int, d: int) -> int:
    """Upper bound of both attention kernels' workspaces (attention_f32x.hip
    nos_attn_f32x6_workspace, attention_h3g.hip nos_attn_h3g_workspace)."""
    skvp = -(-skv // 32) * 32
    return b * max(h, hkv) * skvp * 6 * d * 2 + 4 * b * sq * h * (d + 2) * 4 + b * hkv * (skv // 256 + 2) * 8 + 4096



@dataclass
class Program:
    name: str
    inputs: list[Value]
    params: dict[str, Value]
    param_layout: dict[str, tuple[int, int]]     # name -> (offset, nbytes) in the payload
    nodes: list[Node]
    outputs: list[str]
    values: dict[str, Value]
    payload: bytes | memoryview = b""
    state: dict[str, Value] = field(default_factory=dict)        # persistent buffers (K / V caches, positions)
    state_root: dict[str, str] = field(default_factory=dict)     # a state's in-place versions -> the state
    sampling_state: str | None = None    # the i32 [4] state its ``sample`` nodes read (the server fills it per request)
    stopping_state: str | None = None    # the i32 [8] state its stopping ops read (stop ids, pad id, penalty; per request)
    done_state: str | None = None        # the i32 [B] flags ``done_mark`` sets (a row that drew a stop id)
    seen_state: str | None = None        # the i32 [B, ceil(vocab / 32)] bitmap ``seen_mark`` fills
    speculate_state: str | None = None   # the i32 [4] state ``spec_accept`` reads (the token budget's end; per request)
    hist_state: str | None = None        # the i32 [B, L] token history ``hist_write`` keeps (a speculating tenant)
    adapter_state: str | None = None     # the i32 [B] state its ``lora`` nodes read (an adapter per sequence; per request)

    @property
    def adapters(self) -> int:
        """The adapters n its ``lora`` nodes hold (0: none); the server checks a request's ids against it."""
        return min((self.values[n.inputs[1]].shape[0] for n in self.nodes if n.op == "lora"), default=0)

    # ------------------------------------------------------------ accounting
    @property
    def param_bytes(self) -> int:
        return sum(v.nbytes for v in self.params.values())

    @property
    def state_bytes(self) -> int:
        return sum(v.nbytes for v in self.state.values())

    def is_state(self, name: str) -> bool:
        """A state buffer or one of its in-place versions (the same memory)."""
        return name in self.state or name in self.state_root

    @property
    def bytes_estimate(self) -> int:
        return self.bytes_estimate_for(None)

    def foldable(self) -> set[str]:
        """Node outputs the compiler folds to constants at load time (every
        input a weight or another folded value; never attention)."""
        const = set(self.params)
        out = set()
        for n in self.nodes:
            if n.op not in NEVER_FOLD and all(i in const for i in n.inputs):
                const.add(n.output)
                out.add(n.output)
        return out

    def bytes_estimate_for(self, kernel_config: dict | None = None) -> int:
        """Device bytes a build needs, bounded before anything is allocated:

        * the weights, plus their split planes under the server's fp32 math
          (``kernel_config["f32_math"]``; h3: two fp16 planes = 1x an fp32
          matrix + row scales; x6: three bf16 planes = 1.5x; exact: none) and
          the folded copy LayerNorm / RMSNorm folding makes of a weight
          (+ its two bias vectors);
        * constant-folded values, which are weights too: they are counted as
          persistent (they are materialised at load time and live
          for the tenant's lifetime), never released;
        * the input, and the peak of the unfused graph's live activations
          when every value is released after its last consumer (what the
          compiled program does; fusion only removes intermediates) plus the
          largest per-op workspace live at that point (GEMM A planes, the
          attention's K/V planes, conv im2col planes, ...; :func:`_workspace`),
          twice over: one graph plus the solo graph's private buffers.

        The measured peak of the real build is checked again after it."""
        f32_math = (kernel_config or {}).get("f32_math", "h3")
        folded = self.foldable()
        persistent = sum(self.values[o].nbytes for o in folded)
        last = {}
        for k, n in enumerate(self.nodes):
            for i in n.inputs:
                last[i] = k
        keep = set(self.outputs)
        live = peak = 0
        start = {n.output for n in self.nodes if n.op == "pos_set" and n.attrs.get("value") == 0}
        for k, n in enumerate(self.nodes):
            if n.output in folded:
                continue
            ws = _workspace(n, [self.values[i] for i in n.inputs], self.values[n.output], f32_math)
            # a prefill at position 0 into i8 caches attends the rows the writes hand over dequantized
            # (fp32 copies of K and V, alive from their writes to the attention): charged at all three
            if n.op in ("kv_write", "sdpa_cache"):
                cache, x, p = (1, 0, 3) if n.op == "sdpa_cache" else (0, 1, 2)
                if self.values[n.inputs[cache]].dtype == "i8" and n.inputs[p] in start:
                    b, _, hkv, d = self.values[n.inputs[cache]].shape
                    ws += 2 * b * self.values[n.inputs[x]].shape[1] * hkv * d * 4
            if not self.is_state(n.output):   # an in-place state update allocates nothing
                live += self.values[n.output].nbytes
            peak = max(peak, live + ws)
            for i in set(n.inputs):
                v = self.values[i]
                if (v.kind == "node" and i not in folded and last.get(i) == k and i not in keep
                        and not self.is_state(i)):
                    live -= v.nbytes
        plane_mult = {"h3": 1.0, "x6": 1.5}.get(f32_math, 0.0)
        planes = 0
        by_out = {n.output: n for n in self.nodes}
        for n in self.nodes:
            if n.op not in GEMM_OPS or len(n.inputs) < 2 or n.inputs[1] not in self.params:
                continue
            w = self.values[n.inputs[1]]
            if w.dtype == "fp32":
                planes += int(w.nbytes * plane_mult) + 4 * w.shape[0]
            src = by_out.get(n.inputs[0])
            if src is not None and src.op in ("layernorm", "rmsnorm"):  # the folded copy + c1 / c2
                planes += w.nbytes + 8 * w.shape[0]
        # parallel linears over one activation (Q / K / V, gate / up, heads) are merged into one
        # weight copy by the compiler (not only the norm-fed ones)
        readers: dict[str, list] = {}
        for n in self.nodes:
            if n.op == "linear" and len(n.inputs) >= 2 and n.inputs[1] in self.params:
                readers.setdefault(n.inputs[0], []).append(self.values[n.inputs[1]])
        for ws in readers.values():
            if len(ws) > 1:
                planes += sum(w.nbytes + 4 * w.shape[0] for w in ws)
        # the state (K / V caches, positions) is allocated once, at registration,
        # and never grows at replay: it counts in full against the slice
        return (self.param_bytes + planes + persistent + self.state_bytes + sum(v.nbytes for v in self.inputs)
                + 2 * peak + self.cache_flash_workspace())

    def cache_flash_workspace(self) -> int:
        """The workspace of the flash attention over the K / V caches (``nos_attn_h3g_cache_workspace``: the
        planes of a whole cache, re-split on every call and dropped after it), for the ``sdpa_cache`` nodes
        the compiler's rule moves there (``ops.tenant.cache_flash_rule``) -- once per program (its layers run
        one after the other), 0 without such a node."""
        from ...ops.tenant import cache_flash_rule, sdpa_cache_flash_workspace_bytes

        need = 0
        for n in self.nodes:
            if n.op != "sdpa_cache":
                continue
            q, kc = self.values[n.inputs[0]], self.values[n.inputs[1]]
            (b, sq, h, d), (_, l, hkv, _) = q.shape, kc.shape
            if hkv and h % hkv == 0 and cache_flash_rule(h // hkv, sq, d, q.dtype == "fp32" and kc.dtype == "fp32"):
                need = max(need, sdpa_cache_flash_workspace_bytes(b, h, hkv, sq, l, d))
        return need

    # ------------------------------------------------------------ tensors
    def tensors(self, device) -> dict:
        """The weights as device tensors (copied out of the payload)."""
        import torch

        out = {}
        buf = memoryview(self.payload)
        # the block scales of the MXFP4 linears: one host pass over each, so that no kernel sees a scale byte
        # outside the range it is defined (and tested) on
        mx4_scales = {n.inputs[2] for n in self.nodes if n.op == "linear_mx4"}
        mx4_scales |= {i for n in self.nodes if n.op == "moe_mx4" for i in (n.inputs[3], n.inputs[5])}
        for name, v in self.params.items():
            off, nb = self.param_layout[name]
            raw = np.frombuffer(buf[off:off + nb],
                                dtype={"fp32": np.float32, "i8": np.int8, "u8": np.uint8}.get(v.dtype, np.int16))
            if name in mx4_scales and raw.size and (raw.min() < MX4_SCALE_MIN or raw.max() > MX4_SCALE_MAX):
                bad = int(raw[(raw < MX4_SCALE_MIN) | (raw > MX4_SCALE_MAX)][0])
                raise ValueError(f"param {name!r}: MXFP4 block scale byte {bad} is outside [{MX4_SCALE_MIN}, "
                                 f"{MX4_SCALE_MAX}], the scales whose dequantized values are normal, finite fp32 "
                                 f"(255 is the format's NaN)")
            t = torch.from_numpy(raw.copy()).view(v.shape)
            if v.dtype == "bf16":
                t = t.view(torch.bfloat16)
            out[name] = t.to(device)
        return out

    def state_tensors(self, device) -> dict:
        """The state buffers, zero-initialised (a fresh sequence at position 0)."""
        import torch

        return {k: torch.zeros(v.shape, dtype=torch_dtype(v.dtype), device=device) for k, v in self.state.items()}

    def input_tensor(self, device, data: np.ndarray | None = None):
        import torch

        v = self.inputs[0]
        if data is None:
            x = torch.zeros(v.shape, dtype=torch_dtype(v.dtype))
        elif v.dtype == "i32":
            x = torch.from_numpy(np.ascontiguousarray(data, dtype=np.int32)).view(v.shape)
        else:
            x = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).view(v.shape).to(torch_dtype(v.dtype))
        return x.to(device)

    def id_bound(self) -> int | None:
        """For an i32 (token id) input: the smallest embedding table it
        indexes -- ids must lie in [0, bound) (checked per request)."""
        if self.inputs[0].dtype != "i32":
            return None
        vs = [self.values[n.inputs[1]].shape[0] for n in self.nodes if n.op == "embedding"]
        return min(vs) if vs else None

    # ------------------------------------------------------------ execution
    def compile(self, device, params: dict | None = None, state: dict | None = None,
                derived: dict | None = None) -> "CompiledProgram":  # noqa: F821
        """``state``: the tenant's state tensors (:meth:`state_tensors`), shared
        by every variant compiled over them; None: fresh zero buffers.
        ``derived``: a dict shared by the variants compiled over the same
        ``params`` -- their folded / merged weights are then made once."""
        from .execute import CompiledProgram

        return CompiledProgram(self, device, params, state, derived)

    def reference(self, x, params: dict | None = None, state: dict | None = None) -> tuple:
        """Eager, unfused, fp32 evaluation of the graph on the CPU (the
        numerics reference: every op in plain PyTorch).  ``state``: the
        tenant's state tensors (fp32 / i32 on the CPU), updated in place --
        pass the same dict to consecutive calls (prefill, then decode steps);
        None: a fresh zero state, dropped after the call."""
        import torch

        ps = params if params is not None else self.tensors("cpu")
        env = {k: (t if t.dtype == torch.uint8 else t.float()).cpu() for k, t in ps.items()}
        if state is None:
            state = {k: (t if t.dtype in (torch.int32, torch.int8) else t.float())
                     for k, t in self.state_tensors("cpu").items()}
        env.update(state)
        env[self.inputs[0].name] = x.cpu() if self.inputs[0].dtype == "i32" else x.float().cpu()
        with torch.no_grad():
            for n in self.nodes:
                args = [env[i] for i in n.inputs]
                if n.op == "cast":
                    env[n.output] = args[0]
                else:
                    env[n.output] = _eager(n.op, args, n.attrs, ref=True)
        return tuple(env[o] for o in self.outputs)

