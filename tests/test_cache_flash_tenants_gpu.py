"""Decoder tenants whose multi-token steps run on the flash kernel over their K / V caches
(``stats["flash_cache"]``; compile.py ``_mark_cache_flash``): an ``extend`` chunk of a plain Llama tenant, of a
windowed Mistral tenant whose ring wraps, and a windowed prefill longer than its window -- against the
``transformers`` models in fp64 at the tenants' fp32 logit bar (tests/test_window_gpu.py), with the same tenant
compiled under ``NOS_AMD_CACHE_FLASH=0`` (the decode kernel everywhere) as the fp32 comparison."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402

MAX_LEN = 96


@pytest.fixture(autouse=True)
def _h3():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)


@pytest.fixture(scope="module")
def llama():
    from nos_amd.models.llama_program import llama_config, llama_model

    return llama_model(llama_config(False), 0)        # 2 layers, G = 2, head_dim 128


@pytest.fixture(scope="module")
def mistral():
    from nos_amd.models.llama_program import mistral_config, mistral_model

    return mistral_model(mistral_config(), 0)         # the same shape, sliding window 8


def _compile(model, prompt_len, **kw):
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    progs, w = llama_decode_programs(model, prompt_len, MAX_LEN, **kw)
    ps = PG.parse_variants(progs, w, gpu=True)
    params, state = ps[0].tensors("cuda"), ps[0].state_tensors("cuda")
    return {p.inputs[0].shape[1]: p.compile("cuda", params=params, state=state) for p in ps}, state


def _feed(by_len, ids, plan):
    """Teacher-forced chunks: every chunk's last logits [B, len(plan), V] and the tokens the tenant drew."""
    out, nxt, t = [], [], 0
    with torch.no_grad():
        for n in plan:
            lg, tok = by_len[n](ids[:, t:t + n].cuda())[:2]
            out.append(lg[:, -1:].cpu())
            nxt.append(tok.reshape(-1)[-1:].cpu())
            t += n
    return torch.cat(out, 1), torch.cat(nxt)


def _refs(model, ids, plan):
    rows = (np.cumsum(plan) - 1).tolist()
    with torch.no_grad():
        r64 = copy.deepcopy(model).double()(ids.long()).logits[:, rows]
    return r64, float(r64.abs().max())


def _check(what, got, off, r64, scale):
    """The h3 yardstick (tests/test_tenant_ops_gpu.py ``_close_to_fp64``) on every step's logits: the error
    against fp64 at most max(4 x the decode-path tenant's, 5e-6), relative to max |ref64|."""
    assert bool(torch.isfinite(got).all())
    for i in range(got.shape[1]):
        e = float((got[:, i].double() - r64[:, i]).abs().max()) / scale
        e32 = float((off[:, i].double() - r64[:, i]).abs().max()) / scale
        print(f"{what} step {i}: e = {e:.3g}, decode path e = {e32:.3g}")
        assert e <= max(4 * e32, 5e-6), (what, i, e, e32)


def _off(monkeypatch, model, prompt_len, **kw):
    monkeypatch.setenv("NOS_AMD_CACHE_FLASH", "0")
    try:
        return _compile(model, prompt_len, **kw)
    finally:
        monkeypatch.delenv("NOS_AMD_CACHE_FLASH")


def test_plain_tenant_extends_on_the_flash_kernel(llama, monkeypatch):
    """Prefill 5, one extend of 40, 8 one-token steps on teacher-forced ids."""
    monkeypatch.delenv("NOS_AMD_CACHE_FLASH", raising=False)
    layers = llama.config.num_hidden_layers
    plan = [5, 40] + [1] * 8
    ids = torch.randint(0, 512, (1, sum(plan)), generator=torch.Generator().manual_seed(21), dtype=torch.int32)
    comp, state = _compile(llama, 5, extend=(40,))
    off, off_state = _off(monkeypatch, llama, 5, extend=(40,))
    assert comp[40].stats["flash_cache"] == layers and comp[1].stats["flash_cache"] == 0
    assert off[40].stats["flash_cache"] == 0
    assert comp[1].stats["kernels"] == off[1].stats["kernels"]
    assert [s.kind for s in comp[1].steps] == [s.kind for s in off[1].steps]
    assert sum(s.kind == "kv_write" for s in comp[40].steps) == layers         # the paired kv_write stays a launch
    got, _ = _feed(comp, ids, plan)
    ref, _ = _feed(off, ids, plan)
    assert state["pos"].tolist() == off_state["pos"].tolist() == [sum(plan)]
    r64, scale = _refs(llama, ids, plan)
    _check("llama", got, ref, r64, scale)


def test_plain_tenant_draws_the_tokens_of_generate(llama, monkeypatch):
    """A 45-token prompt fed as prefill 5 + extend 40, then greedy one-token steps on the tenant's own tokens."""
    monkeypatch.delenv("NOS_AMD_CACHE_FLASH", raising=False)
    prompt = torch.randint(0, 512, (1, 45), generator=torch.Generator().manual_seed(22), dtype=torch.int32)
    with torch.no_grad():
        want = llama.generate(prompt.long(), max_new_tokens=9, min_new_tokens=9, do_sample=False, pad_token_id=0)[0, 45:]
        full = torch.cat([prompt.long(), want[None]], 1)
        r64 = copy.deepcopy(llama).double()(full).logits[0, 44:53]
        r32 = llama(full).logits[0, 44:53]
    top = r64.topk(2, dim=-1).values
    err = (r32.double() - r64).abs().amax(-1)
    assert bool((top[:, 0] - top[:, 1] > 4 * err).all()), "a near-tie in the reference"
    comp, state = _compile(llama, 5, extend=(40,))
    toks = []
    with torch.no_grad():
        comp[5](prompt[:, :5].cuda())
        tok = comp[40](prompt[:, 5:].cuda())[1]
        for _ in range(9):
            toks.append(int(tok.reshape(-1)[-1]))
            tok = comp[1](tok.reshape(1, 1).int())[1]
    assert toks == want.tolist(), (toks, want.tolist())


def test_flash_extend_replays_in_a_captured_graph(llama, monkeypatch):
    """Nothing on the host reads the positions: the extend step captured once at position 5 replays there bit
    for bit, and again at position 45 (the counter moved on the device) as the eager step does there."""
    monkeypatch.delenv("NOS_AMD_CACHE_FLASH", raising=False)
    ids = torch.randint(0, 512, (1, 85), generator=torch.Generator().manual_seed(23), dtype=torch.int32)
    comp, state = _compile(llama, 5, extend=(40,))
    x = ids[:, 5:45].cuda()
    with torch.no_grad():
        comp[5](ids[:, :5].cuda())
        saved = {k: v.clone() for k, v in state.items()}
        eager1 = comp[40](x)[0].clone()
        x.copy_(ids[:, 45:85])
        eager2 = comp[40](x)[0].clone()
        for k, v in state.items():
            v.copy_(saved[k])
        x.copy_(ids[:, 5:45])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = comp[40](x)[0]
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager1)
        x.copy_(ids[:, 45:85])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager2)
    assert state["pos"].tolist() == [85]
    assert not torch.equal(eager1, eager2)


def test_windowed_tenant_extends_on_the_flash_kernel(mistral, monkeypatch):
    """Window 8, extend 40: a ring of 47 slots; prefill 5, two extends and 8 one-token steps end at position 93:
    the ring wraps.  Against ``MistralForCausalLM`` in fp64."""
    monkeypatch.delenv("NOS_AMD_CACHE_FLASH", raising=False)
    layers = mistral.config.num_hidden_layers
    plan = [5, 40, 40] + [1] * 8
    ids = torch.randint(0, 512, (1, sum(plan)), generator=torch.Generator().manual_seed(24), dtype=torch.int32)
    comp, state = _compile(mistral, 5, extend=(40,))
    off, _ = _off(monkeypatch, mistral, 5, extend=(40,))
    assert state["kc0"].shape[1] == 8 + 40 - 1 < sum(plan)
    assert comp[40].stats["flash_cache"] == layers and comp[1].stats["flash_cache"] == 0
    assert comp[40].stats["ring_caches"] == 2 * layers
    got, _ = _feed(comp, ids, plan)
    ref, _ = _feed(off, ids, plan)
    assert state["pos"].tolist() == [sum(plan)]
    r64, scale = _refs(mistral, ids, plan)
    _check("mistral", got, ref, r64, scale)


def test_long_windowed_prefill_runs_on_the_flash_kernel(mistral, monkeypatch):
    """prompt_len 44 > window 8: the static prefill stays a ``sdpa_cache`` over the ring (every row sees its
    last 8 keys among the step's own) and moves to the flash kernel."""
    monkeypatch.delenv("NOS_AMD_CACHE_FLASH", raising=False)
    layers = mistral.config.num_hidden_layers
    plan = [44] + [1] * 8
    ids = torch.randint(0, 512, (1, sum(plan)), generator=torch.Generator().manual_seed(25), dtype=torch.int32)
    comp, state = _compile(mistral, 44)
    off, _ = _off(monkeypatch, mistral, 44)
    assert comp[44].stats["flash_cache"] == layers and comp[1].stats["flash_cache"] == 0
    assert off[44].stats["flash_cache"] == 0
    got, _ = _feed(comp, ids, plan)
    ref, _ = _feed(off, ids, plan)
    r64, scale = _refs(mistral, ids, plan)
    _check("mistral long prefill", got, ref, r64, scale)
