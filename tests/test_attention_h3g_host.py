"""Host side of the general h3 attention, without a GPU: the argument checks of
``nos_attn_h3g``, ``nos_attn_h3g_lse`` and ``nos_attn_h3g_bwd`` (every
rejection returns before any HIP call, so the built library is all they need)
and the two workspace functions."""
from __future__ import annotations

import pytest

INVALID = 1  # hipErrorInvalidValue
B, H, HKV, S, D = 1, 2, 1, 33, 64
LD = 512      # token row stride of every operand: room for the head counts and head dims the defects set
BIG = 1 << 30  # workspace bytes of the rows that change a dimension: their one defect is the dimension
FWD, LSE, BWD = "nos_attn_h3g", "nos_attn_h3g_lse", "nos_attn_h3g_bwd"


def _p(i: int) -> int:
    """A dummy 256-byte aligned device pointer (nothing is dereferenced)."""
    return 0x100000 * (i + 1)


def _rows(name: str, ld: str, bs: str, i: int) -> dict:
    return {name: _p(i), ld: LD, bs: S * LD}


@pytest.fixture(scope="module")
def lib():
    from nos_amd.ops import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def valid(lib):
    """One valid argument set per entry point, in the order of the C signature (ops/_lib.py:_SIGS)."""
    qkv = {**_rows("q", "ldq", "bsq", 0), **_rows("k", "ldk", "bsk", 1), **_rows("v", "ldv", "bsv", 2),
           **_rows("o", "ldo", "bso", 3)}
    dims = dict(B=B, H=H, Hkv=HKV, Sq=S, Skv=S, D=D, causal=0, scale=0.125)
    fwd = {**qkv, **dims, "rope_cos": None, "rope_sin": None, "rope_bound": 0.0, "ws": _p(9),
           "ws_bytes": lib.nos_attn_h3g_workspace(B, H, HKV, S, S, D)}
    bwd = {**qkv, **_rows("dout", "lddo", "bsdo", 4), "lse": _p(10), **_rows("dq", "lddq", "bsdq", 5),
           **_rows("dk", "lddk", "bsdk", 6), **_rows("dv", "lddv", "bsdv", 7), **dims, "ws": _p(9),
           "ws_bytes": lib.nos_attn_h3g_bwd_workspace(B, H, HKV, S, S, D), "stream": None}
    assert fwd["ws_bytes"] > 0 and bwd["ws_bytes"] > 0
    return {FWD: {**fwd, "stream": None}, LSE: {**fwd, "lse": _p(10), "stream": None}, BWD: bwd}


ALL, FWDS, TRAIN = (FWD, LSE, BWD), (FWD, LSE), (LSE, BWD)
# (entry points, defect, the arguments that carry it -- everything else stays valid; "ws_bytes": -1 = one byte short).
# "[new]": the forwards used to launch on these (a null pointer passed their alignment test); the backward never did.
DEFECTS = [
    (ALL, "B = 0", dict(B=0, ws_bytes=BIG)),
    (ALL, "H % Hkv", dict(Hkv=3, ws_bytes=BIG)),
    (ALL, "D = 96", dict(D=96, ws_bytes=BIG)),
    (ALL, "scale = 0", dict(scale=0.0)),
    (ALL, "causal with Sq > Skv", dict(causal=1, Sq=S + 1, ws_bytes=BIG)),
    (ALL, "ldq < H * D", dict(ldq=H * D - 4)),
    (ALL, "ldk < Hkv * D", dict(ldk=HKV * D - 4)),
    (ALL, "ldq % 4", dict(ldq=H * D + 2)),
    (ALL, "bsq % 4", dict(bsq=S * LD + 2)),
    (ALL, "q not 16-byte aligned", dict(q=_p(0) + 8)),
    (ALL, "workspace not 256-byte aligned", dict(ws=_p(9) + 16)),
    (ALL, "workspace null", dict(ws=None)),
    (ALL, "workspace one byte short", dict(ws_bytes=-1)),
    (FWDS, "cos table without sin", dict(rope_cos=_p(11), rope_bound=2.0)),
    (FWDS, "tables with rope_bound = 0", dict(rope_cos=_p(11), rope_sin=_p(12), rope_bound=0.0)),
    (FWDS, "rope with Sq > Skv", dict(rope_cos=_p(11), rope_sin=_p(12), rope_bound=2.0, Sq=S + 1, ws_bytes=BIG)),
    (TRAIN, "lse null", dict(lse=None)),
    (TRAIN, "lse not 4-byte aligned", dict(lse=_p(10) + 2)),
    (FWDS, "q null [new]", dict(q=None)),
    (FWDS, "k null [new]", dict(k=None)),
    (FWDS, "v null [new]", dict(v=None)),
    (FWDS, "o null [new]", dict(o=None)),
    *(((BWD,), f"{name} null", {name: None}) for name in ("q", "k", "v", "o", "dout", "dq", "dk", "dv")),
    ((BWD,), "lddo < H * D", dict(lddo=H * D - 4)),
]
ROWS = [(fn, what, bad) for fns, what, bad in DEFECTS for fn in fns]


@pytest.mark.parametrize("fn,what,bad", ROWS, ids=[f"{fn[9:]}-{what}" for fn, what, _ in ROWS])
def test_h3g_attention_entry_rejects(lib, valid, fn, what, bad):
    assert set(bad) <= set(valid[fn]), "a defect names arguments of the entry point"
    args = {**valid[fn], **bad}
    if bad.get("ws_bytes") == -1:
        args["ws_bytes"] = valid[fn]["ws_bytes"] - 1
    assert getattr(lib, fn)(*args.values()) == INVALID


def test_h3g_attention_workspace_functions_reject_bad_dims(lib):
    for ws in (lib.nos_attn_h3g_workspace, lib.nos_attn_h3g_bwd_workspace):
        assert ws(B, H, HKV, S, S, 96) == -1
        assert ws(0, H, HKV, S, S, D) == -1
    assert lib.nos_attn_h3g_bwd_workspace(B, H, 3, S, S, D) == -1
    # the forward's function has never checked the grouping: its sizes need H and Hkv, not H / Hkv
    assert lib.nos_attn_h3g_workspace(B, H, 3, S, S, D) > 0
