"""Chunked prefill on the flash kernel, without a GPU: the compiler's rule (``ops.tenant.cache_flash_rule``,
``Lowered._mark_cache_flash``), its environment switch, ``sdpa_cache(flash=)`` on CPU tensors, the memory
estimate's workspace term and the host checks of ``nos_attn_h3g_cache`` / ``nos_attn_h3g_cache_ring`` (every
rejection returns before any HIP call, so the built library is all they need)."""
from __future__ import annotations

import pytest
import torch

from nos_amd.ops import tenant as T
from nos_amd.podserver.program.reference import sdpa_cache_ref

INVALID = 1   # hipErrorInvalidValue
MAX_LEN = 96


def test_the_rule_is_more_rows_than_one_decode_pass():
    assert T.DECODE_MAX_ROWS == 32
    for G, Sq, want in ((4, 8, False), (4, 9, True), (2, 16, False), (2, 17, True), (1, 32, False), (1, 33, True),
                        (32, 1, False), (8, 1, False)):
        assert T.cache_flash_rule(G, Sq, 128, True, env={}) is want, (G, Sq)
    assert T.cache_flash_rule(4, 64, 64, True, env={}) and not T.cache_flash_rule(4, 64, 96, True, env={})
    assert not T.cache_flash_rule(4, 64, 128, False, env={})                      # a bf16 tenant, int8 caches
    assert not T.cache_flash_rule(4, 64, 128, True, env={"NOS_AMD_CACHE_FLASH": "0"})
    assert T.cache_flash_rule(4, 64, 128, True, env={"NOS_AMD_CACHE_FLASH": "1"})


def _variants(model, prompt_len, **kw):
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    progs, w = llama_decode_programs(model, prompt_len, MAX_LEN, **kw)
    ps = PG.parse_variants(progs, w, gpu=False)
    params, state = ps[0].tensors("cpu"), ps[0].state_tensors("cpu")
    return ps, {p.inputs[0].shape[1]: p.compile("cpu", params=params, state=state) for p in ps}


@pytest.fixture(scope="module")
def llama():
    from nos_amd.models.llama_program import llama_config, llama_model

    return llama_model(llama_config(False), 0)       # G = 2, head_dim 128


@pytest.fixture(scope="module")
def mistral():
    from nos_amd.models.llama_program import mistral_config, mistral_model

    return mistral_model(mistral_config(), 0)         # G = 2, head_dim 128, window 8


def _flash_steps(c):
    return [s for s in c.steps if s.kind == "sdpa_cache" and s.attrs.get("flash")]


def test_the_compiler_marks_the_steps_over_the_rule(llama, mistral, monkeypatch):
    monkeypatch.delenv("NOS_AMD_CACHE_FLASH", raising=False)
    layers = llama.config.num_hidden_layers
    _, c = _variants(llama, 5, extend=(16, 40))
    assert c[40].stats["flash_cache"] == layers == len(_flash_steps(c[40]))
    for n in (1, 5, 16):      # the one-token step, the static prefill (causal sdpa), G x Sq = 32
        assert c[n].stats["flash_cache"] == 0 and not _flash_steps(c[n])
    for s in _flash_steps(c[40]):
        assert not s.attrs.get("fresh") and not s.attrs.get("sync") and not s.attrs.get("partials")
    assert sum(s.kind == "kv_write" for s in c[40].steps) == layers     # the paired write stays a launch
    _, cw = _variants(mistral, 5, extend=(40,))
    assert cw[40].stats["flash_cache"] == layers and cw[1].stats["flash_cache"] == 0
    assert all(s.attrs["window"] == 8 and s.attrs["limit"] == MAX_LEN for s in _flash_steps(cw[40]))
    _, cl = _variants(mistral, 44)       # the long windowed prefill: static positions leave it a sdpa_cache
    assert cl[44].stats["flash_cache"] == layers and cl[1].stats["flash_cache"] == 0
    for kw in (dict(dtype="bf16"), dict(kv="int8")):      # they keep the decode kernel
        _, cb = _variants(llama, 5, extend=(40,), **kw)
        assert cb[40].stats["flash_cache"] == 0 and not _flash_steps(cb[40])


def test_the_environment_switch_keeps_the_decode_path(llama, monkeypatch):
    monkeypatch.setenv("NOS_AMD_CACHE_FLASH", "0")
    ps, c = _variants(llama, 5, extend=(40,))
    assert c[40].stats["flash_cache"] == 0 and not _flash_steps(c[40])
    assert all(p.cache_flash_workspace() == 0 for p in ps)


def test_the_estimate_grows_by_the_workspace(llama, monkeypatch):
    from nos_amd.ops import _lib

    monkeypatch.delenv("NOS_AMD_CACHE_FLASH", raising=False)
    ps, _ = _variants(llama, 5, extend=(40,))
    ext = next(p for p in ps if p.inputs[0].shape[1] == 40)
    one = next(p for p in ps if p.inputs[0].shape[1] == 1)
    cfg = llama.config
    H, Hkv, D = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.hidden_size // cfg.num_attention_heads
    need = T.sdpa_cache_flash_workspace_bytes(1, H, Hkv, 40, MAX_LEN, D)
    assert need == _lib.lib().nos_attn_h3g_cache_workspace(1, H, Hkv, 40, MAX_LEN, D) > 0
    with_flash, one_with = ext.bytes_estimate, one.bytes_estimate
    monkeypatch.setenv("NOS_AMD_CACHE_FLASH", "0")
    assert with_flash - ext.bytes_estimate == need
    assert one_with == one.bytes_estimate
    for shape in ((2, 8, 2, 290, 700, 64), (3, 4, 4, 33, 33, 128), (1, 8, 1, 256, 8192, 128)):
        assert T.sdpa_cache_flash_workspace_bytes(*shape) == _lib.lib().nos_attn_h3g_cache_workspace(*shape)


@pytest.mark.parametrize("kw", [dict(), dict(window=8, limit=64)])
def test_flash_on_cpu_tensors_is_the_reference(kw):
    g = torch.Generator().manual_seed(3)
    q = torch.randn(2, 5, 4, 64, generator=g)
    kc, vc = torch.randn(2, 12, 2, 64, generator=g), torch.randn(2, 12, 2, 64, generator=g)
    kx, vx = torch.randn(2, 5, 2, 64, generator=g), torch.randn(2, 5, 2, 64, generator=g)
    pos = torch.tensor([0, 6], dtype=torch.int32)
    outs = {}
    for flash in (True, False, None):
        k, v = kc.clone(), vc.clone()
        outs[flash] = (T.sdpa_cache(q, k, v, pos, fresh=(kx, vx), flash=flash, **kw), k, v)
    for flash in (True, None):
        assert all(torch.equal(a, b) for a, b in zip(outs[flash], outs[False]))
    assert torch.equal(outs[True][0], sdpa_cache_ref(q, outs[True][1], outs[True][2], pos, **kw))


def test_the_entry_points_check_their_arguments():
    from nos_amd.ops import _lib

    lib = _lib.lib()
    p = lambda i: 0x100000 * (i + 1)     # dummy aligned device pointers: nothing is dereferenced
    B, H, Hkv, Sq, L, D = 1, 4, 2, 5, 12, 128

    def call(ring=None, **bad):
        a = dict(q=p(0), ldq=H * D, bsq=Sq * H * D, kc=p(1), vc=p(2), pos=p(3), cos=None, sin=None, R=0, o=p(4),
                 ldo=H * D, bso=Sq * H * D, B=B, H=H, Hkv=Hkv, Sq=Sq, L=L, D=D, scale=0.1, ws=p(9), ws_bytes=1 << 30)
        a.update(bad)
        if ring is not None:
            return lib.nos_attn_h3g_cache_ring(*a.values(), ring[0], ring[1], None)
        return lib.nos_attn_h3g_cache(*a.values(), None)

    for bad in (dict(D=96), dict(Hkv=3), dict(B=0), dict(scale=0.0), dict(pos=None), dict(kc=None), dict(vc=p(2) + 8),
                dict(q=None), dict(o=None), dict(ws=None), dict(ws=p(9) + 16), dict(cos=p(5)), dict(cos=p(5), sin=p(6), R=0),
                dict(ws_bytes=lib.nos_attn_h3g_cache_workspace(B, H, Hkv, Sq, L, D) - 1), dict(ldq=H * D - 4)):
        assert call(**bad) == INVALID, bad
        assert call(ring=(8, 64), **bad) == INVALID, bad
    # the ring's own checks (nos_attn_decode_ring's): min(limit, W + Sq - 1) <= C <= limit, Sq <= C, limit <= R
    for ring, bad in (((8, 64), dict(L=11)), ((0, 64), {}), ((8, 0), {}), ((8, 11), {}), ((8, 64), dict(Sq=13, L=12)),
                      ((8, 64), dict(cos=p(5), sin=p(6), R=63))):
        assert call(ring=ring, **bad) == INVALID, (ring, bad)
    assert lib.nos_attn_h3g_cache_workspace(B, H, Hkv, Sq, L, 96) == -1
