"""Decoder-LLM tenants: a ``transformers`` Llama as a pod-server program.

The MPS clients of the reference are arbitrary CUDA programs
(``/root/reference/docs/en/docs/dynamic-gpu-partitioning/partitioning-modes-comparison.md:29-34``);
this builder makes the canonical decoder LLM one: a random-init
``LlamaForCausalLM`` (no checkpoints: there is no network) is written as the
program op graph -- token-id input, embedding gather, per layer RMSNorm ->
Q / K / V projections -> rotary -> causal grouped-query attention -> output
projection + residual -> RMSNorm -> SwiGLU MLP + residual, final RMSNorm and
the LM head -- with the module's own weights, so the program's logits are
compared against the HF module's forward (tests/test_llama_tenant.py, GPU:
tests/test_tenant_programs_gpu.py).  On the server the compiler merges the
Q / K / V (and gate / up) projections into one GEMM each, folds every
RMSNorm into the GEMM after it (``linear_rms``), moves the rotary embedding
into the attention (``nos_attn_h3g``: causal, head_dim 128, GQA) and the
residual adds into GEMM epilogues.

The rotary tables are the HF default rope (``rope_theta``, no scaling) for
positions 0..S-1, computed in float64 and stored as fp32 weights.
"""
from __future__ import annotations

import numpy as np

from ..podserver.program import (Builder, dequantize_rows_mx4, dequantize_rows_q8, quantize_rows_mx4,
                                 quantize_rows_q8)

# the HF Llama linears an int8 tenant stores quantized (every weight but the embedding table and the norms)
_Q8_LINEARS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def llama_config(small: bool = True, **kw):
    """A LlamaConfig: ``small`` -- the fleet tenant (1024 hidden, 8 layers,
    8 heads of 128, 2 KV heads, 2816 MLP, 32000 vocab); else the tests' tiny
    variant.  Keyword arguments override fields."""
    from transformers import LlamaConfig

    base = dict(hidden_size=1024, num_hidden_layers=8, num_attention_heads=8, num_key_value_heads=2,
                intermediate_size=2816, vocab_size=32000, max_position_embeddings=4096, rms_norm_eps=1e-5,
                rope_theta=10000.0, tie_word_embeddings=False) if small else \
        dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
             intermediate_size=512, vocab_size=512, max_position_embeddings=512, rms_norm_eps=1e-5,
             rope_theta=10000.0, tie_word_embeddings=False)
    base.update(kw)
    return LlamaConfig(**base)


def llama_model(cfg, seed: int = 0):
    """A random-init HF LlamaForCausalLM in fp32, eval mode (eager attention)."""
    import torch
    from transformers import LlamaForCausalLM

    torch.manual_seed(seed)
    cfg._attn_implementation = "eager"
    m = LlamaForCausalLM(cfg).float().eval()
    with torch.no_grad():  # non-trivial norm weights (HF initialises them to ones)
        g = torch.Generator().manual_seed(seed + 1)
        for name, p in m.named_parameters():
            if name.endswith("norm.weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
    return m


def mixtral_config(small: bool = True, **kw):
    """A MixtralConfig: ``small`` -- the tests' tiny variant (4 experts, top-2); else the fleet shape, the
    fleet Llama tenant with its MLP as E = 8 experts of ``intermediate_size`` 1408 and k = 2, so a token
    streams the dense fleet decoder's MLP bytes.  Keyword arguments override fields."""
    from transformers import MixtralConfig

    base = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                intermediate_size=96, vocab_size=512, max_position_embeddings=512, rms_norm_eps=1e-5,
                num_local_experts=4, num_experts_per_tok=2, sliding_window=None, tie_word_embeddings=False) if small else \
        dict(hidden_size=1024, num_hidden_layers=8, num_attention_heads=8, num_key_value_heads=2,
             intermediate_size=1408, vocab_size=32000, max_position_embeddings=4096, rms_norm_eps=1e-5,
             num_local_experts=8, num_experts_per_tok=2, sliding_window=None, tie_word_embeddings=False)
    base.update(kw)
    return MixtralConfig(**base)


def mixtral_model(cfg, seed: int = 0):
    """A random-init HF MixtralForCausalLM in fp32, eval mode (eager attention); the router's weights are
    drawn at three times HF's 0.02, so that the experts' probabilities differ clearly and no expert's is tiny."""
    import torch
    from transformers import MixtralForCausalLM

    torch.manual_seed(seed)
    cfg._attn_implementation = "eager"
    cfg._experts_implementation = "eager"   # the per-expert loop (any dtype; the grouped GEMM takes no fp64)
    m = MixtralForCausalLM(cfg).float().eval()
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 1)
        for name, p in m.named_parameters():
            if name.endswith("norm.weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith("mlp.gate.weight"):
                p.copy_(0.06 * torch.randn(p.shape, generator=g))
    return m


def mistral_config(small: bool = True, **kw):
    """A MistralConfig: ``small`` -- the tests' tiny variant (sliding window 8); else the fleet decoder's shape
    with a window of 1024.  Keyword arguments override fields."""
    from transformers import MistralConfig

    base = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                intermediate_size=512, vocab_size=512, max_position_embeddings=512, rms_norm_eps=1e-5,
                sliding_window=8, tie_word_embeddings=False) if small else \
        dict(hidden_size=1024, num_hidden_layers=8, num_attention_heads=8, num_key_value_heads=2,
             intermediate_size=2816, vocab_size=32000, max_position_embeddings=8192, rms_norm_eps=1e-5,
             sliding_window=1024, tie_word_embeddings=False)
    base.update(kw)
    return MistralConfig(**base)


def mistral_model(cfg, seed: int = 0):
    """A random-init HF MistralForCausalLM in fp32, eval mode (eager attention)."""
    import torch
    from transformers import MistralForCausalLM

    torch.manual_seed(seed)
    cfg._attn_implementation = "eager"
    m = MistralForCausalLM(cfg).float().eval()
    with torch.no_grad():  # non-trivial norm weights (HF initialises them to ones)
        g = torch.Generator().manual_seed(seed + 1)
        for name, p in m.named_parameters():
            if name.endswith("norm.weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
    return m


def _rope_theta(cfg) -> float:
    """The rotary base: ``rope_parameters["rope_theta"]`` where the config keeps it there (transformers 5),
    else its ``rope_theta`` attribute, else 10000."""
    rp = getattr(cfg, "rope_parameters", None)
    if isinstance(rp, dict) and rp.get("rope_theta") is not None:
        return float(rp["rope_theta"])
    return float(getattr(cfg, "rope_theta", 10000.0))


def rope_tables(seq: int, head_dim: int, theta: float) -> tuple[np.ndarray, np.ndarray]:
    inv = 1.0 / theta ** (np.arange(0, head_dim, 2, dtype=np.float64) / head_dim)
    f = np.outer(np.arange(seq, dtype=np.float64), inv)
    emb = np.concatenate([f, f], axis=1)
    return np.cos(emb).astype(np.float32), np.sin(emb).astype(np.float32)


def llama_program(model, seq: int, batch: int = 1, dtype: str = "fp32",
                  rope_len: int | None = None) -> tuple[dict, bytes]:
    """(program, weights) of causal-LM logits [batch, seq, vocab] for token
    ids [batch, seq] (i32).  ``rope_len`` (>= seq): the rotary tables' rows
    in the weights, sliced to ``seq`` in the graph (folded at load) -- the
    programs of several sequence lengths then share one weight payload (the
    pod server's shape variants)."""
    rope_len = seq if rope_len is None else rope_len
    if rope_len < seq:
        raise ValueError(f"rope_len {rope_len} < seq {seq}")
    cfg = model.config
    sd = {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()}
    d, nh = cfg.hidden_size, cfg.num_attention_heads
    nkv = cfg.num_key_value_heads
    hd = getattr(cfg, "head_dim", None) or d // nh
    eps = float(cfg.rms_norm_eps)
    b = Builder(f"llama-h{d}-l{cfg.num_hidden_layers}-{dtype}")
    ids = b.input("input_ids", [batch, seq], "i32")
    P = lambda k: b.param(k, sd[k], dtype)  # noqa: E731
    cos, sin = rope_tables(rope_len, hd, _rope_theta(cfg))
    rc, rs = b.param("rope.cos", cos, "fp32"), b.param("rope.sin", sin, "fp32")
    if rope_len > seq:
        rc, rs = (b.op("slice", t, dim=0, start=0, end=seq) for t in (rc, rs))
    h = b.op("embedding", ids, P("model.embed_tokens.weight"))
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        y = b.op("rmsnorm", h, P(p + "input_layernorm.weight"), eps=eps)
        q = b.op("reshape", b.op("linear", y, P(p + "self_attn.q_proj.weight")), shape=[batch, seq, nh, hd])
        k = b.op("reshape", b.op("linear", y, P(p + "self_attn.k_proj.weight")), shape=[batch, seq, nkv, hd])
        v = b.op("reshape", b.op("linear", y, P(p + "self_attn.v_proj.weight")), shape=[batch, seq, nkv, hd])
        q, k = b.op("rotary", q, rc, rs), b.op("rotary", k, rc, rs)
        o = b.op("reshape", b.op("sdpa", q, k, v, causal=True), shape=[batch, seq, nh * hd])
        h = b.op("add", b.op("linear", o, P(p + "self_attn.o_proj.weight")), h)
        y = b.op("rmsnorm", h, P(p + "post_attention_layernorm.weight"), eps=eps)
        g = b.op("linear", y, P(p + "mlp.gate_proj.weight"))
        u = b.op("linear", y, P(p + "mlp.up_proj.weight"))
        h = b.op("add", b.op("linear", b.op("mul", b.op("silu", g), u), P(p + "mlp.down_proj.weight")), h)
    h = b.op("rmsnorm", h, P("model.norm.weight"), eps=eps)
    head = "lm_head.weight" if "lm_head.weight" in sd else "model.embed_tokens.weight"
    logits = b.op("linear", h, P(head), out="logits")
    return b.build([logits])


# the projections an adapter may target, grouped by the activation they read: a group's adapters are
# stacked into ONE lora node (its A rows [A_q; A_k; A_v], its B block-structured over the merged columns)
_LORA_GROUPS = (("self_attn.qkv_proj", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")),
                ("self_attn.o_proj", ("self_attn.o_proj",)),
                ("mlp.gate_up_proj", ("mlp.gate_proj", "mlp.up_proj")),
                ("mlp.down_proj", ("mlp.down_proj",)))
LORA_MAX_RANK = 64   # the stacked rank of one activation (ops.tenant.LORA_MAX_RANK)


def _stack_adapters(adapters, model) -> dict:
    """``adapters`` (a list of {module name: (A [r, in], B [out, r], scale)}) checked and stacked per
    adapted activation: {``model.layers.i.<group>``: (A [n, R, in], B [n, N, R], member modules)} with
    N the merged projections' output columns, R = r x (targeted members), ``scale`` folded into B and
    zero blocks where a member is not targeted or a column belongs to another member."""
    cfg = model.config
    if not isinstance(adapters, (list, tuple)) or not adapters or not all(isinstance(a, dict) and a for a in adapters):
        raise ValueError("adapters must be a non-empty list of {module name: (A, B, scale)} dicts")
    sd = model.state_dict()
    valid = {f"model.layers.{i}.{m}" for i in range(cfg.num_hidden_layers) for _, ms in _LORA_GROUPS for m in ms}
    targets = set(adapters[0])
    rank = None
    for k, ad in enumerate(adapters):
        unknown = sorted(set(ad) - valid)
        if unknown:
            raise ValueError(f"adapters[{k}]: unknown module name {unknown[0]!r}; an adapter targets "
                             f"model.layers.<i>.self_attn.{{q,k,v,o}}_proj and model.layers.<i>.mlp.{{gate,up,down}}_proj")
        if set(ad) != targets:
            raise ValueError(f"adapters[{k}] targets other modules than adapters[0]: all adapters of one tenant share "
                             f"one target set (differing: {sorted(set(ad) ^ targets)[:4]})")
        for name, (A, B, _scale) in ad.items():
            w = sd[name + ".weight"]
            A, B = np.asarray(A), np.asarray(B)
            if A.ndim != 2 or B.ndim != 2 or A.shape[1] != w.shape[1] or B.shape[0] != w.shape[0] or B.shape[1] != A.shape[0]:
                raise ValueError(f"adapters[{k}][{name!r}]: A [r, {w.shape[1]}] and B [{w.shape[0]}, r] required, got "
                                 f"{A.shape} and {B.shape}")
            if rank not in (None, A.shape[0]):
                raise ValueError(f"adapters[{k}][{name!r}] has rank {A.shape[0]}, others {rank}: all adapters of one "
                                 f"tenant share one rank")
            rank = A.shape[0]
    out = {}
    for i in range(cfg.num_hidden_layers):
        for group, members in _LORA_GROUPS:
            hit = [m for m in members if f"model.layers.{i}.{m}" in targets]
            if not hit:
                continue
            R = rank * len(hit)
            if R > LORA_MAX_RANK or R % 4:
                raise ValueError(f"model.layers.{i}.{group}: the stacked rank R = {rank} x {len(hit)} = {R} must be a "
                                 f"multiple of 4 and at most {LORA_MAX_RANK} (the adapters of the projections that read "
                                 f"one activation are stacked)")
            widths = [sd[f"model.layers.{i}.{m}.weight"].shape[0] for m in members]
            K = sd[f"model.layers.{i}.{members[0]}.weight"].shape[1]
            As = np.zeros((len(adapters), R, K), np.float32)
            Bs = np.zeros((len(adapters), sum(widths), R), np.float32)
            for k, ad in enumerate(adapters):
                for j, m in enumerate(hit):
                    A, B, scale = ad[f"model.layers.{i}.{m}"]
                    row = sum(widths[:members.index(m)])
                    As[k, j * rank:(j + 1) * rank] = np.asarray(A, np.float32)
                    Bs[k, row:row + widths[members.index(m)], j * rank:(j + 1) * rank] = \
                        np.float32(scale) * np.asarray(B, np.float32)
            out[f"model.layers.{i}.{group}"] = (As, Bs, members)
    return out


def llama_decode_programs(model, prompt_len: int, max_len: int, batch: int = 1, dtype: str = "fp32",
                          extend: tuple[int, ...] = (), sampling: bool = False,
                          weights: str = "fp32", kv: str | None = None,
                          stopping: bool = False, speculate: int | None = None,
                          adapters: list | None = None, window: int | None = None,
                          experts: str = "fp32") -> tuple[list[dict], bytes]:
    """A STATEFUL generation tenant: ``[prefill, decode, *extends]`` programs
    over one weight payload and one state -- per layer a K and a V cache
    ``[batch, max_len, kv_heads, head_dim]`` plus the position counter
    ``pos`` [batch] (i32) -- registered as shape variants (the server routes
    by the input's shape):

    * prefill, input ids ``[batch, prompt_len]``: starts a sequence
      (``pos_set`` 0), writes the prompt's K / V into the caches, attends
      causally (the compiler sees position 0 and runs the flash kernel on the
      fresh keys), advances ``pos`` by ``prompt_len``;
    * decode, input ids ``[batch, 1]``: one token at the device-side position
      -- rotary at ``pos``, ``kv_write`` of its K / V, ``sdpa_cache`` over the
      cache (decode.hip), ``pos`` += 1;
    * ``extend`` lengths: like decode for chunks of that many tokens (a longer
      prompt = prefill + extends + decode steps).

    Every program outputs the last token's logits ``[batch, 1, vocab]`` and
    the greedy next ids ``[batch, 1]`` (i32, ``argmax``), so a client's
    generation loop sends back one id per step.  The caches' bytes count
    against the slice at registration; a replay never allocates state.

    ``sampling``: the programs also declare the control state ``sampling``
    (i32 [4], filled by the server from each request's ``"sampling"`` field)
    and end in ``sample`` instead of ``argmax``: the next ids are drawn under
    the request's temperature / top-k / top-p / seed, keyed on the position
    before the step's advance (the prefill draws at counter 0, the decode
    steps at ``prompt_len``, ``prompt_len`` + 1, ...); a request without
    sampling parameters stays greedy.

    ``weights="int8"`` (fp32 tenants): every linear's weight is stored as int8
    rows with one fp32 scale per output row (``Builder.param_q8``) and read by
    ``linear_q8`` nodes -- q / k / v merged into one weight, o, gate / up
    merged, down and the LM head (its own quantized copy when the head is
    tied; the embedding table stays fp32).  Quantization is a storage format:
    the server computes, in fp32, exactly the model
    :func:`dequantized_llama` returns.

    ``weights="mxfp4"`` (fp32 tenants): the same linears stored as OCP Microscaling MXFP4
    (``Builder.param_mx4``: 4-bit E2M1 codes, one E8M0 scale byte per 32 consecutive inputs of a row,
    4.25 bits a weight) and read by ``linear_mx4`` nodes, merged as for int8 (blocks run along the
    inputs, so merging rows and quantizing commute).  A storage format again:
    ``dequantized_llama(model, weights="mxfp4")`` is the model the server computes.  It combines with
    ``batch``, ``extend``, ``sampling``, ``stopping``, ``kv="int8"``, ``window`` and ``speculate`` (under the
    int8 staging rule below); refused, each with its rule: ``dtype="bf16"``, ``adapters`` (no adapter
    epilogue on the MXFP4 GEMV yet), a Mixtral (no quantized experts yet) and a hidden or
    intermediate size that is no multiple of 32.

    ``kv="int8"`` (fp32 tenants; default: the tenant's dtype): the caches are
    i8 states ``kc{i}`` / ``vc{i}`` with one fp32 scale per (sequence,
    position, KV head) row in ``ks{i}`` / ``vs{i}`` ``[batch, max_len,
    kv_heads]`` -- a quarter of the fp32 caches' bytes plus the scales.  Here
    the server does quantize: every K (after its rotation) and V row as it is
    written, by ``quantize_rows_q8``'s rule, and every program attends the
    rows as the cache holds them -- an HF model run with
    :func:`kv_q8_roundtrip_cache` is the model such a tenant computes.

    ``stopping`` (any dtype, with or without the options above): generation
    that ends, with transformers' ``generate(eos_token_id=[...],
    pad_token_id=..., repetition_penalty=...)`` semantics, all on the device.
    The programs also declare ``done`` (i32 [batch]: the row has emitted a stop
    id), ``seen`` (i32 [batch, ceil(vocab / 32)]: the bitmap of the ids the
    row's sequence holds, prompt and fed-back ids) and the control state
    ``stopping`` (i32 [8], filled by the server from each request's
    ``"stopping"`` field: up to four stop ids, a pad id, a repetition
    penalty).  Every program marks its input ids (the prefill clears the
    bitmaps and ``done`` first), draws from the penalised logits (the
    ``logits`` output stays raw) and closes with ``pos_add(pos, done)`` ->
    ``stop_ids`` -> ``done_mark``: a row's counter advances in every step it
    entered unfinished (the one that emits its stop id included), the stop id
    itself is emitted and every later id of the row is the pad id, and a
    finished row's counter -- so its cache rows below it -- never changes
    again.  All-zero control words (a request without the field): exactly the
    plain tenant's tokens.

    ``speculate=K`` (2 <= K <= 8; fp32 tenants, greedy, without stopping):
    greedy speculative decoding with n-gram drafts looked up in the
    sequence's own history -- the plain tenant's tokens in fewer steps.  The
    programs also declare ``hist`` (i32 [batch, max_len]: ``hist[b, t]`` is the
    token at position t for every t <= ``pos[b]``; ``hist[b, pos[b]]`` is the
    pending token, drawn but not yet through the model) and the control state
    ``speculate`` (i32 [4]: ``[end, 0, 0, 0]``, filled by the server from each
    request's ``"speculate"`` field; no step advances a counter past ``end`` >
    0).  Every program keeps ``hist`` true (its input ids at ``pos + s``, the
    drawn id at the new ``pos``), the prefill also outputs ``spec_ids``
    [batch, K] (the pending token and K - 1 drafts), and a VERIFY program
    ``[batch, K]`` joins the variants: the extend-K body with the LM head on
    all K rows, ``g = argmax(logits)``, then ``spec_accept`` (the drafts the
    model confirmed, plus one), ``hist_write``, ``pos_advance`` and
    ``spec_draft``.  Its outputs are ``logits`` [batch, K, vocab], ``next_ids``
    [batch, K] (the next verify step's input) and ``n_acc`` [batch] (the
    positions the step advanced).  The K / V rows a step wrote past the accepted
    ones are never attended: attention reads keys up to its own position, and
    the rows are rewritten (int8 caches: with their scales) when those
    positions are processed.  With ``weights="int8"`` the verify step's rows must
    also fit the int8 GEMV's staging (``batch * K * widest in-features * 4 <=
    GEMV_X_BYTES``), so that no linear dequantizes a transient weight; an fp32
    tenant past that bound is built, and that linear runs on the fp32 GEMM
    instead of the GEMV (slower: docs/tenant_programs.md).

    ``adapters`` (fp32 tenants; with every option above): N LoRA fine-tunes of
    the model as ONE tenant -- the base weights once, and per adapter a dict
    from module name (``model.layers.{i}.self_attn.q_proj``, ..., ``mlp.down_proj``:
    any subset of q k v o gate up down, the same for every adapter, at one
    rank) to ``(A [r, in], B [out, r], scale)``.  The programs also declare the
    control state ``adapter`` (i32 [batch], filled by the server from each
    request's ``"adapter"`` field: the adapter of each sequence, 1 .. N; 0: the
    base model) and hold ``add(linear(x, W), lora(x, A, B, adapter))`` for
    every adapted activation -- q / k / v (and gate / up) as one merged linear
    with one stacked A ``[A_q; A_k; A_v]`` and a B block-structured over the
    merged columns (``scale`` folded in, zero blocks stored), the stacked rank
    at most 64 and a multiple of 4.  :func:`adapted_llama` is the model such a
    tenant computes for one adapter.  Adapters are fixed at registration.

    A ``MixtralForCausalLM`` (``config.model_type == "mixtral"``) builds the same
    programs, named ``mixtral-...``, with the MLP half of every layer as ``h =
    add(moe(rmsnorm(h), mlp.gate.weight, mlp.experts.gate_up_proj,
    mlp.experts.down_proj, top_k=num_experts_per_tok), h)`` over the fused expert
    tensors as the state dict holds them.  ``batch``, ``extend``, ``sampling``,
    ``stopping``, ``kv="int8"``, ``speculate`` and ``adapters`` on q / k / v / o work
    as above; refused, each with its rule: ``weights="int8"`` / ``"mxfp4"`` (quantized
    experts are ``experts=``, below), ``dtype="bf16"``,
    adapter targets in the MLP, a ``sliding_window`` smaller than ``max_len`` and a
    ``speculate`` with ``batch * K * max(H, I) * 4 > GEMV_X_BYTES``.

    ``experts="int8"`` / ``"mxfp4"`` (a Mixtral only; default ``"fp32"``): the two expert tensors of every
    layer are stored quantized -- ``Builder.param_q8`` / ``param_mx4`` of the 3-D tensors, row by row over
    the last axis (block by block for MXFP4) -- and read by ``moe_q8`` / ``moe_mx4`` nodes; the programs are
    named ``...-fp32-eq8-...`` / ``...-fp32-emx4-...``.  The attention linears, the LM head, the embedding
    and the router stay fp32 (routing is discontinuous, and the router is E x H floats).  A storage format,
    as ``weights=`` is for a dense model: the server computes, in fp32, exactly
    ``dequantized_llama(model, experts=...)``.  It combines with everything a Mixtral takes (``batch``,
    ``extend``, ``sampling``, ``stopping``, ``kv="int8"``, ``speculate``, ``adapters`` on q / k / v / o);
    refused: ``dtype="bf16"``, and a hidden or intermediate size that is no multiple of 16 (int8) or 32
    (MXFP4).  ``experts="fp32"`` programs are byte for byte those built without the keyword.

    ``window`` (default: ``config.sliding_window`` of a ``MistralForCausalLM``, else none; with every
    option above): sliding-window attention, the query at position p attending the W positions
    max(0, p - W + 1) .. p.  It takes effect only for W < ``max_len`` (else the programs are the plain
    ones, byte for byte).  The caches are then RINGS of ``C = min(max_len, W + S - 1)`` slots, S the
    longest step of the tenant (``prompt_len``, the ``extend`` lengths, ``speculate``): position p
    lives in slot p % C, a step writes its rows and then attends, and the row a fresh row replaces
    lies outside every window of the step and of every later one -- a verify step's rejected rows
    included.  ``kv_write`` and ``sdpa_cache`` carry ``window=W, limit=max_len``; ``hist``, the rotary
    tables and the server's context limit stay at ``max_len``, so the caches cost C rows whatever
    ``max_len`` is.  A prompt longer than W keeps the decode kernel for its prefill (correct, slow:
    docs/tenant_programs.md).  A Mixtral takes no window."""
    from ..ops.tenant import GEMV_MAX_ROWS, GEMV_X_BYTES

    moe = getattr(model.config, "model_type", None) == "mixtral"
    if experts not in ("fp32", "int8", "mxfp4"):
        raise ValueError(f"experts must be 'fp32', 'int8' or 'mxfp4', got {experts!r}")
    if experts != "fp32" and not moe:
        raise ValueError(f"experts={experts!r} is a Mixtral tenant's option (the storage format of its expert tensors): "
                         f"this model has no experts; a dense model's linears are quantized with weights=")
    if moe:
        _refuse_mixtral(model.config, max_len, batch, dtype, weights, speculate, adapters, GEMV_X_BYTES)
        if window is not None:
            raise ValueError("a Mixtral tenant takes no window (no sliding-window attention beside the moe op yet)")
        if experts != "fp32":
            mult, what = (16, "16 int8 weights are one 16-byte load") if experts == "int8" else \
                (32, "an MXFP4 block is 32 consecutive inputs of an expert row under one scale byte")
            for name, size in (("hidden_size", model.config.hidden_size),
                               ("intermediate_size", model.config.intermediate_size)):
                if size % mult:
                    raise ValueError(f"experts={experts!r}: {name} = {size} is not a multiple of {mult} ({what})")
    if window is None and getattr(model.config, "model_type", None) == "mistral":
        window = getattr(model.config, "sliding_window", None)
    if window is not None and (not isinstance(window, int) or isinstance(window, bool) or window < 1):
        raise ValueError(f"window must be an int >= 1 (the positions a query attends, itself included), got {window!r}")
    if adapters is not None and dtype != "fp32":
        raise ValueError("adapters are an fp32 tenant's (fp32 A and B beside fp32 or int8 weights): dtype must be 'fp32', "
                         "dtype='bf16' is not taken")
    stacked = _stack_adapters(adapters, model) if adapters is not None else {}

    if speculate is not None:
        if not isinstance(speculate, int) or isinstance(speculate, bool) or not 2 <= speculate <= 8:
            raise ValueError(f"speculate must be an int in [2, 8] (the tokens a verify step takes), got {speculate!r}")
        if batch * speculate > GEMV_MAX_ROWS:
            raise ValueError(f"speculate: batch * K = {batch * speculate} > {GEMV_MAX_ROWS} (GEMV_MAX_ROWS): every "
                             f"linear of the verify step must stay one GEMV launch")
        widest = max(model.config.hidden_size, model.config.intermediate_size)
        if weights in ("int8", "mxfp4") and batch * speculate * widest * 4 > GEMV_X_BYTES:
            raise ValueError(f"speculate: batch * K = {batch * speculate} rows of {widest} inputs are more than the "
                             f"{'int8' if weights == 'int8' else 'MXFP4'} "
                             f"GEMV stages ({GEMV_X_BYTES} bytes of x rows): that linear of the verify step would "
                             f"dequantize a transient fp32 weight")
        if dtype != "fp32":
            raise ValueError("speculate: dtype must be 'fp32' (a K-row and a 1-row bf16 step may round a near-tie "
                             "differently; the contract is token equality)")
        if sampling or stopping:
            raise ValueError("speculate: greedy only -- sampling=True and stopping=True do not combine with it")
        if speculate in (prompt_len, *extend):
            raise ValueError(f"speculate: K = {speculate} is also the prompt length or an extend length; "
                             f"the server routes variants by input shape")
    if not 0 < prompt_len <= max_len:
        raise ValueError(f"prompt_len must be in [1, {max_len}]")
    if weights not in ("fp32", "int8", "mxfp4"):
        raise ValueError(f"weights must be 'fp32', 'int8' or 'mxfp4', got {weights!r}")
    if weights == "int8" and dtype != "fp32":
        raise ValueError("int8 weights are an fp32 tenant's storage format: dtype must be 'fp32'")
    if weights == "mxfp4":
        if dtype != "fp32":
            raise ValueError("MXFP4 weights are an fp32 tenant's storage format: dtype must be 'fp32', dtype='bf16' is "
                             "not taken")
        if adapters is not None:
            raise ValueError("adapters do not combine with weights='mxfp4': the MXFP4 GEMV has no adapter epilogue yet "
                             "(fp32 and int8 weights take adapters)")
        for what, size in (("hidden_size", model.config.hidden_size),
                           ("intermediate_size", model.config.intermediate_size)):
            if size % 32:
                raise ValueError(f"weights='mxfp4': {what} = {size} is not a multiple of 32 (an MXFP4 block is 32 "
                                 f"consecutive inputs of a linear under one scale byte)")
    if kv not in (None, "fp32", "int8") or (kv == "fp32" and dtype != "fp32"):
        raise ValueError(f"kv must be None (the tenant's dtype), 'fp32' (fp32 tenants) or 'int8', got {kv!r}")
    if kv == "int8" and dtype != "fp32":
        raise ValueError("int8 K / V caches are an fp32 tenant's storage format: dtype must be 'fp32'")
    q8, mx4, kvq8 = weights == "int8", weights == "mxfp4", kv == "int8"
    quant = q8 or mx4   # a quantized tenant: q / k / v and gate / up merged by the builder, the head a copy of its own
    cfg = model.config
    sd = {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()}
    d, nh = cfg.hidden_size, cfg.num_attention_heads
    nkv = cfg.num_key_value_heads
    hd = getattr(cfg, "head_dim", None) or d // nh
    eps = float(cfg.rms_norm_eps)
    cos, sin = rope_tables(max_len, hd, _rope_theta(cfg))
    head = "lm_head.weight" if "lm_head.weight" in sd else "model.embed_tokens.weight"
    cache_dt = "bf16" if dtype == "bf16" else "fp32"
    progs = []
    chunks = [(prompt_len, True, False), (1, False, False)] + [(n, False, False) for n in extend]
    if speculate:
        chunks.append((speculate, False, True))
    # a window below max_len: every variant's caches are one ring, sized for the longest step
    ring_slots = min(max_len, window + max(n for n, _, _ in chunks) - 1) if window is not None and window < max_len \
        else None
    ring = {"window": window, "limit": max_len} if ring_slots else {}
    payload = b""
    for seq, reset, verify in chunks:
        b = Builder(f"{'mixtral' if moe else 'llama'}-h{d}-l{cfg.num_hidden_layers}-{dtype}{'-q8' if q8 else '-mx4' if mx4 else ''}{'-eq8' if experts == 'int8' else '-emx4' if experts == 'mxfp4' else ''}{'-kvq8' if kvq8 else ''}-"
                    f"{'stop-' if stopping else ''}{'spec-' if speculate else ''}{'lora-' if stacked else ''}"
                    f"{'prefill' if reset else 'verify' if verify else 'step'}{seq}")
        ids = b.input("input_ids", [batch, seq], "i32")
        P = lambda k: b.param(k, sd[k], dtype)  # noqa: E731

        def lin(x, name, *keys, out=None):
            """x @ W^T: a ``linear`` over the weight ``name``; for int8 weights a ``linear_q8`` (MXFP4: a
            ``linear_mx4``) over the rows of ``keys``' weights (default: ``name``'s), merged and then
            quantized -- with a scale per row (per block of a row) that equals quantizing each and
            merging, so no compiler pass has to merge."""
            if not quant:
                return b.op("linear", x, P(name), out=out)
            w = np.concatenate([sd[k] for k in keys or (name,)], axis=0)
            wq, sc = b.param_mx4(name, w) if mx4 else b.param_q8(name, w)
            return b.op("linear_mx4" if mx4 else "linear_q8", x, wq, sc, out=out)

        def adapted(y, x, group):
            """y (the group's merged linear of x) plus its adapters' delta, where the group has any."""
            if group not in stacked:
                return y
            As, Bs, _ = stacked[group]
            return b.op("add", y, b.op("lora", x, b.param(group + ".lora_A", As), b.param(group + ".lora_B", Bs), sel))

        def merged(x, group):
            """An adapted group's projections as ONE linear over the members' rows (the arrangement int8
            weights use): merging and adapters commute, so the delta is added to the merged output."""
            keys = [group.rsplit(".", 2)[0] + "." + m + ".weight" for m in stacked[group][2]]
            if quant or len(keys) == 1:
                return lin(x, group + ".weight" if len(keys) > 1 else keys[0], *(keys if len(keys) > 1 else ()))
            return b.op("linear", x, b.param(group + ".weight", np.concatenate([sd[k] for k in keys], axis=0), dtype))

        rc, rs = b.param("rope.cos", cos, "fp32"), b.param("rope.sin", sin, "fp32")
        b.state("pos", [batch], "i32")
        sel = b.adapter_state(batch) if stacked else None
        ctl = b.state("sampling", [4], "i32") if sampling else None
        done, seen, sctl = b.stopping_states(batch, cfg.vocab_size) if stopping else (None, None, None)
        hist, spec_ctl = b.speculate_states(batch, max_len) if speculate else (None, None)
        cshape = [batch, ring_slots or max_len, nkv, hd]
        if kvq8:   # ((K cache, its scales), (V cache, its scales)) per layer
            caches = [(b.cache_q8(f"kc{i}", f"ks{i}", cshape), b.cache_q8(f"vc{i}", f"vs{i}", cshape))
                      for i in range(cfg.num_hidden_layers)]
        else:
            caches = [((b.state(f"kc{i}", cshape, cache_dt),), (b.state(f"vc{i}", cshape, cache_dt),))
                      for i in range(cfg.num_hidden_layers)]
        p = b.op("pos_set", "pos", value=0) if reset else "pos"
        h = b.op("embedding", ids, P("model.embed_tokens.weight"))
        for i in range(cfg.num_hidden_layers):
            pf = f"model.layers.{i}."
            y = b.op("rmsnorm", h, P(pf + "input_layernorm.weight"), eps=eps)
            if quant or pf + "self_attn.qkv_proj" in stacked:
                if pf + "self_attn.qkv_proj" in stacked:
                    qkv = adapted(merged(y, pf + "self_attn.qkv_proj"), y, pf + "self_attn.qkv_proj")
                else:
                    qkv = lin(y, pf + "self_attn.qkv_proj.weight", *(pf + f"self_attn.{t}_proj.weight" for t in "qkv"))
                ends = (0, nh * hd, (nh + nkv) * hd, (nh + 2 * nkv) * hd)
                proj = lambda t: b.op("slice", qkv, dim=-1, start=ends[t], end=ends[t + 1])  # noqa: E731
            else:
                proj = lambda t: b.op("linear", y, P(pf + f"self_attn.{'qkv'[t]}_proj.weight"))  # noqa: E731
            q = b.op("reshape", proj(0), shape=[batch, seq, nh, hd])
            k = b.op("reshape", proj(1), shape=[batch, seq, nkv, hd])
            v = b.op("reshape", proj(2), shape=[batch, seq, nkv, hd])
            q, k = b.op("rotary_at", q, rc, rs, p), b.op("rotary_at", k, rc, rs, p)
            (kc0, *ks), (vc0, *vs) = caches[i]   # ks / vs: the scales states of i8 caches, else empty
            kc = b.op("kv_write", kc0, k, p, *ks, **ring)
            vc = b.op("kv_write", vc0, v, p, *vs, **ring)
            o = b.op("reshape", b.op("sdpa_cache", q, kc, vc, p, *ks, *vs, **ring), shape=[batch, seq, nh * hd])
            h = b.op("add", adapted(lin(o, pf + "self_attn.o_proj.weight"), o, pf + "self_attn.o_proj"), h)
            y = b.op("rmsnorm", h, P(pf + "post_attention_layernorm.weight"), eps=eps)
            if moe:   # the sparse MLP: the router, the fused expert tensors as the state dict holds them
                egu, edn = pf + "mlp.experts.gate_up_proj", pf + "mlp.experts.down_proj"
                if experts == "fp32":
                    h = b.op("add", b.moe(y, P(pf + "mlp.gate.weight"), P(egu), P(edn), cfg.num_experts_per_tok), h)
                    continue
                # quantized experts: codes and scales of the two tensors; the router stays fp32
                quantized = b.param_q8 if experts == "int8" else b.param_mx4
                node = b.moe_q8 if experts == "int8" else b.moe_mx4
                h = b.op("add", node(y, P(pf + "mlp.gate.weight"), *quantized(egu, sd[egu]), *quantized(edn, sd[edn]),
                                     cfg.num_experts_per_tok), h)
                continue
            if quant or pf + "mlp.gate_up_proj" in stacked:
                if pf + "mlp.gate_up_proj" in stacked:
                    gu = adapted(merged(y, pf + "mlp.gate_up_proj"), y, pf + "mlp.gate_up_proj")
                else:
                    gu = lin(y, pf + "mlp.gate_up_proj.weight", pf + "mlp.gate_proj.weight", pf + "mlp.up_proj.weight")
                inter = sd[pf + "mlp.gate_proj.weight"].shape[0]
                g = b.op("slice", gu, dim=-1, start=0, end=inter)
                u = b.op("slice", gu, dim=-1, start=inter, end=2 * inter)
            else:
                g = b.op("linear", y, P(pf + "mlp.gate_proj.weight"))
                u = b.op("linear", y, P(pf + "mlp.up_proj.weight"))
            act = b.op("mul", b.op("silu", g), u)
            h = b.op("add", adapted(lin(act, pf + "mlp.down_proj.weight"), act, pf + "mlp.down_proj"), h)
        if seq > 1 and not verify:   # only the last token's logits: the LM head runs on one row
            h = b.op("slice", h, dim=1, start=seq - 1, end=seq)
        h = b.op("rmsnorm", h, P("model.norm.weight"), eps=eps)
        # a tied head reads the embedding table: quantized, it is a copy of its own (the table stays fp32)
        logits = lin(h, "lm_head.weight", head, out="logits") if quant else lin(h, head, out="logits")
        if verify:
            # the draw after every row, the drafts it confirms (+ 1), the history and the counter
            # advanced by that many, and the next step's input: the new pending token and its drafts
            g = b.op("argmax", logits)
            acc = b.op("spec_accept", ids, g, p, spec_ctl, out="n_acc", limit=max_len)
            hv = b.op("hist_write", hist, p, ids, g, acc, lead=1)
            nxt = b.op("spec_draft", hv, b.op("pos_advance", p, acc), out="next_ids", k=speculate)
            prog, w = b.build([logits, nxt, acc])
            progs.append(prog)
            payload = w
            continue
        if stopping:
            # the input ids join the row's bitmap, the seen tokens' logits are penalised (the ``logits``
            # output stays raw), then the draw; a finished row emits the pad id and keeps its counter,
            # and a row that emits a stop id is finished from the next step on
            dn = b.op("pos_set", done, value=0) if reset else done
            pen = b.op("penalize", logits, b.op("seen_mark", seen, ids, reset=reset), sctl)
            raw = b.op("sample", pen, ctl, p) if sampling else b.op("argmax", pen)
            b.op("pos_add", p, dn, n=seq)
            nxt = b.op("stop_ids", raw, dn, sctl, out="next_ids")
            b.op("done_mark", dn, nxt, sctl)
        else:
            nxt = b.op("sample", logits, ctl, p, out="next_ids") if sampling else b.op("argmax", logits, out="next_ids")
            p2 = b.op("pos_add", p, n=seq)
        outs = [logits, nxt]
        if speculate:   # the history: the input ids at pos .. pos + seq - 1, the drawn id at the new pos
            hv = b.op("hist_write", hist, p2, ids, nxt, back=seq)
            if reset:
                outs.append(b.op("spec_draft", hv, p2, out="spec_ids", k=speculate))
        prog, w = b.build(outs)
        progs.append(prog)
        payload = w
    return progs, payload


def _refuse_mixtral(cfg, max_len, batch, dtype, weights, speculate, adapters, x_bytes) -> None:
    """What a Mixtral tenant does not take (``llama_decode_programs``), each with its rule."""
    if weights in ("int8", "mxfp4"):
        raise ValueError(f"a Mixtral tenant's weights are fp32: weights={weights!r} is not taken (no quantized experts "
                         f"yet)")
    if dtype != "fp32":
        raise ValueError(f"a Mixtral tenant is fp32 (the moe op takes an fp32 x and fp32 experts): dtype={dtype!r} "
                         f"is not taken")
    if adapters is not None:
        mlp = sorted(k for a in adapters if isinstance(a, dict) for k in a if ".mlp." in str(k))
        if mlp:
            raise ValueError(f"a Mixtral tenant's adapters target q / k / v / o only: {mlp[0]!r} is in the MLP, which "
                             f"is a mixture of experts")
    sw = getattr(cfg, "sliding_window", None)
    if sw is not None and sw < max_len:
        raise ValueError(f"sliding_window = {sw} is set and smaller than max_len = {max_len}: the caches attend every "
                         f"earlier position (no sliding-window attention here)")
    if isinstance(speculate, int) and not isinstance(speculate, bool):
        widest = max(cfg.hidden_size, cfg.intermediate_size)
        if batch * speculate * widest * 4 > x_bytes:
            raise ValueError(f"speculate: batch * K * max(H, I) * 4 = {batch * speculate * widest * 4} > {x_bytes} "
                             f"(GEMV_X_BYTES): the verify step's rows must fit the staging of the GEMVs and the moe "
                             f"kernels")


def dequantized_llama(model, weights: str = "int8", experts: str | None = None):
    """A deep copy of the HF model whose linear weights (attention and MLP
    projections, the LM head -- untied from the embedding table, which stays
    fp32) are ``dequantize(quantize(w))`` row by row (``weights="mxfp4"``: block
    by block, ``quantize_rows_mx4``): the model an int8 (MXFP4) tenant of
    ``model`` computes (``llama_decode_programs(weights=...)``), for tests and
    users to compare against.

    ``experts="int8"`` / ``"mxfp4"`` (a Mixtral): instead, ONLY the expert tensors
    ``mlp.experts.gate_up_proj`` and ``mlp.experts.down_proj`` are round-tripped, row by row over the
    last axis (``quantize_rows_q8`` / ``quantize_rows_mx4`` on the tensor flattened to [E * N, K]);
    everything else keeps its fp32 values: the model a tenant built with
    ``llama_decode_programs(experts=...)`` computes."""
    if experts is not None:
        if experts not in ("int8", "mxfp4"):
            raise ValueError(f"dequantized_llama: experts must be 'int8' or 'mxfp4', got {experts!r}")
        import copy

        import torch

        rt = ((lambda w: dequantize_rows_mx4(*quantize_rows_mx4(w))) if experts == "mxfp4"
              else (lambda w: dequantize_rows_q8(*quantize_rows_q8(w))))
        m = copy.deepcopy(model)
        with torch.no_grad():
            for name, p in m.named_parameters():
                if name.endswith(("mlp.experts.gate_up_proj", "mlp.experts.down_proj")):
                    w = p.detach().float().cpu().numpy()
                    p.copy_(torch.from_numpy(rt(w.reshape(-1, w.shape[-1])).reshape(w.shape)).to(p.dtype))
        return m
    if weights not in ("int8", "mxfp4"):
        raise ValueError(f"dequantized_llama: weights must be 'int8' or 'mxfp4', got {weights!r}")
    roundtrip = ((lambda w: dequantize_rows_mx4(*quantize_rows_mx4(w))) if weights == "mxfp4"
                 else (lambda w: dequantize_rows_q8(*quantize_rows_q8(w))))
    import copy

    import torch

    m = copy.deepcopy(model)
    with torch.no_grad():
        head = m.lm_head.weight.detach().float().cpu().numpy()
        if m.lm_head.weight.data_ptr() == m.model.embed_tokens.weight.data_ptr():   # tied: the head gets its own copy
            m.config.tie_word_embeddings = False
            m.lm_head.weight = torch.nn.Parameter(m.lm_head.weight.detach().clone())
        for name, p in m.named_parameters():
            if name == "lm_head.weight" or (name.endswith("_proj.weight") and name.split(".")[-2] in _Q8_LINEARS):
                w = head if name == "lm_head.weight" else p.detach().float().cpu().numpy()
                p.copy_(torch.from_numpy(roundtrip(w)).to(p.dtype))
    return m


def adapted_llama(model, adapter: dict):
    """A deep copy of the HF model whose targeted ``nn.Linear`` modules (``adapter``: {module name:
    (A [r, in], B [out, r], scale)}) compute ``base(x) + scale * (x @ A.T) @ B.T``, unmerged and in
    that order of operations: the model an adapter tenant computes for the sequences that select this
    adapter (``llama_decode_programs(adapters=[...])``), for tests and users to compare against."""
    import copy

    import torch

    class LoraLinear(torch.nn.Module):
        def __init__(self, base, A, B, scale):
            super().__init__()
            self.base, self.scale = base, float(scale)
            self.lora_A = torch.nn.Parameter(torch.as_tensor(np.asarray(A, np.float32)).to(base.weight.dtype), False)
            self.lora_B = torch.nn.Parameter(torch.as_tensor(np.asarray(B, np.float32)).to(base.weight.dtype), False)

        def forward(self, x):
            return self.base(x) + self.scale * ((x @ self.lora_A.T) @ self.lora_B.T)

    m = copy.deepcopy(model)
    for name, (A, B, scale) in adapter.items():
        parent, _, leaf = name.rpartition(".")
        base = m.get_submodule(name)
        if not isinstance(base, torch.nn.Linear):
            raise ValueError(f"adapted_llama: {name!r} is no nn.Linear of the model")
        setattr(m.get_submodule(parent), leaf, LoraLinear(base, A, B, scale))
    return m.eval()


def kv_q8_roundtrip_cache():
    """A ``transformers`` cache for ``model(..., past_key_values=...)`` whose
    ``update()`` replaces the incoming K (already rotated) and V by
    ``dequantize(quantize(.))`` -- per token and KV head, in fp32, by
    ``quantize_rows_q8``'s rule -- and stores and returns those: an HF model
    run with it is the model an int8-KV tenant computes
    (``llama_decode_programs(kv="int8")``), for tests and users to compare against."""
    import torch
    from transformers import DynamicCache

    def roundtrip(x):   # [B, Hkv, S, D]
        rows = x.detach().to(torch.float32).cpu().reshape(-1, x.shape[-1]).numpy()
        deq = torch.from_numpy(dequantize_rows_q8(*quantize_rows_q8(rows)))
        return deq.reshape(x.shape).to(device=x.device, dtype=x.dtype)

    class KvQ8RoundtripCache(DynamicCache):
        def update(self, key_states, value_states, layer_idx, cache_kwargs=None):
            return super().update(roundtrip(key_states), roundtrip(value_states), layer_idx, cache_kwargs)

    return KvQ8RoundtripCache()


def llama_tenant(dtype: str = "fp32", seed: int = 0, small: bool = True, seq: int = 512,
                 batch: int = 1) -> tuple[dict, bytes]:
    """(program, weights) of the decoder-LLM tenant (``small=False``: the
    tiny test config at seq 64)."""
    m = llama_model(llama_config(small), seed)
    return llama_program(m, seq if small else 64, batch, dtype)


__all__ = ["mistral_config", "mistral_model", "mixtral_config", "mixtral_model", "llama_config", "llama_model", "llama_program", "llama_decode_programs", "llama_tenant", "rope_tables",
           "dequantized_llama", "kv_q8_roundtrip_cache", "adapted_llama"]
