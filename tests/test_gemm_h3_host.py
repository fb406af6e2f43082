"""Host side of the h3 GEMMs, without a GPU: the argument checks of the four
``nos_gemm_f32h3*`` entry points (every rejection returns before any HIP
call, so the built library is all they need) and ``ops.apply_kernel_config``."""
from __future__ import annotations

import pytest

INVALID = 1  # hipErrorInvalidValue
EPI_BIAS, EPI_RESID, EPI_BIAS_ROW, EPI_RESID_PRE = 1, 4, 16, 32
M, N, K = 128, 192, 64  # N / 3 = 64: also a valid fused QKV projection


def _p(i: int) -> int:
    """A dummy 16-byte aligned device pointer (nothing is dereferenced)."""
    return 0x100000 * (i + 1)


# one valid argument set per entry point, in the order of the C signature (ops/_lib.py:_SIGS)
_OPERANDS = dict(Wp=_p(2), ldw=K, wplane=N * K, csc=_p(3), bias=_p(4), R=_p(5), ldr=N, C=_p(6), ldc=N, M=M, N=N, K=K,
                 epi=0)
_A_PLANES = dict(Ap=_p(0), lda=K, aplane=M * K, rinv=_p(1), rconst=1.0)
_OUTPUTS = dict(kvs=None, S=0, skvp=0, kvsc=None, P=None, ldp=0, pplane=0, psc=1.0)
VALID = {
    "nos_gemm_f32h3": {**_A_PLANES, **_OPERANDS, **_OUTPUTS, "stream": None},
    "nos_gemm_f32h3_stats": {**_A_PLANES, **_OPERANDS, "stats": _p(7), "stream": None},
    "nos_gemm_f32h3_lna": {"X": _p(0), "ldx": K, "stats": _p(7), "nparts": 1, "pw": K, "eps": 1e-5, "eln": 3,
                           **_OPERANDS, **_OUTPUTS, "stream": None},
    "nos_gemm_f32h3_batched": dict(Ap=_p(0), lda=K, aplane=M * K, sa=2 * M * K, rinv=_p(1), srinv=M, rconst=1.0,
                                   Wp=_p(2), ldw=K, wplane=N * K, sw=2 * N * K, csc=_p(3), scsc=N, bias=_p(4), sbias=N,
                                   R=_p(5), ldr=N, sr=M * N, C=_p(6), ldc=N, sc=M * N, M=M, N=N, K=K, nb=3, epi=0,
                                   stream=None),
}
GEMM, STATS, LNA, BATCHED = VALID

_KV = dict(kvs=_p(8), kvsc=_p(9), S=M, skvp=M)  # a valid K / V plane output
_PLANES = dict(P=_p(10), ldp=N, pplane=M * N)   # a valid plane output (psc from the base set)
# (entry points, defect, the arguments that carry it -- everything else stays valid)
DEFECTS = [
    ((GEMM, STATS, BATCHED, LNA), "K % 32", dict(K=48)),
    ((GEMM, STATS, BATCHED), "lda < K", dict(lda=56, aplane=M * 56)),
    ((GEMM, STATS, BATCHED), "lda % 8", dict(lda=68, aplane=M * 68)),
    ((GEMM, STATS, BATCHED), "aplane < M * lda", dict(aplane=M * K - 8)),
    ((GEMM, STATS, BATCHED), "Ap not 16-byte aligned", dict(Ap=_p(0) + 8)),
    ((GEMM, STATS, BATCHED, LNA), "csc null", dict(csc=None)),
    ((GEMM, STATS, BATCHED, LNA), "EPI_BIAS without bias", dict(epi=EPI_BIAS, bias=None)),
    ((GEMM, STATS, BATCHED, LNA), "EPI_RESID with ldr < N", dict(epi=EPI_RESID, ldr=N - 4)),
    ((GEMM, STATS, LNA), "EPI_RESID_PRE on a non-batched entry", dict(epi=EPI_RESID_PRE)),
    ((BATCHED,), "both bias flags", dict(epi=EPI_BIAS | EPI_BIAS_ROW)),
    ((BATCHED,), "negative batch stride of A", dict(sa=-8)),
    ((BATCHED,), "negative batch stride of the bias", dict(sbias=-1)),
    ((BATCHED,), "overlapping batched outputs", dict(sc=(M - 1) * N + N - 1)),
    ((GEMM, LNA), "kvs with N % 3", dict(_KV, N=196, wplane=196 * K, ldr=196, ldc=196)),
    ((GEMM, LNA), "kvs with (N / 3) % 64", dict(_KV, N=288, wplane=288 * K, ldr=288, ldc=288)),
    ((GEMM, LNA), "kvs with M % S", dict(_KV, S=48, skvp=64)),
    ((GEMM, LNA), "kvs with skvp below the padded key count", dict(_KV, S=16, skvp=16)),  # whole 32-key tiles: 32
    ((GEMM, LNA), "kvs with skvp above the padded key count", dict(_KV, S=16, skvp=64)),
    ((GEMM, LNA), "kvs together with P", dict(_KV, **_PLANES)),
    ((GEMM, LNA), "psc <= 0", dict(_PLANES, psc=0.0)),
    ((STATS,), "N % 4", dict(N=190)),
    ((LNA,), "nparts * pw < K", dict(nparts=1, pw=32)),
    ((LNA,), "(nparts - 1) * pw >= K", dict(nparts=2, pw=K)),
]
ROWS = [(fn, what, bad) for fns, what, bad in DEFECTS for fn in fns]


@pytest.fixture(scope="module")
def lib():
    from nos_amd.ops import _lib

    return _lib.lib()


@pytest.mark.parametrize("fn,what,bad", ROWS, ids=[f"{fn[4:]}-{what}" for fn, what, _ in ROWS])
def test_h3_gemm_entry_rejects(lib, fn, what, bad):
    assert set(bad) <= set(VALID[fn]), "a defect names arguments of the entry point"
    args = {**VALID[fn], **bad}
    assert getattr(lib, fn)(*args.values()) == INVALID


def test_retired_h3_switches_are_gone_from_the_library(lib):
    """The A/B switches whose variants lost (docs/kernels.md) have no entry
    point left; the statistics part width defaults to 128."""
    for name in ("nos_gemm_f32h3_set_layout", "nos_gemm_f32h3_set_lna_wide", "nos_attn_f32h3_set_waves"):
        assert not hasattr(lib, name), name
    assert lib.nos_gemm_f32h3_hot_bn() == 128
    # the two switches that remain still refuse unknown codes
    assert lib.nos_gemm_f32h3_set_hot_bn(96) == INVALID
    assert lib.nos_gemm_f32h3_set_hot_ring(4) == INVALID


# ------------------------------------------------------- apply_kernel_config
class _Recorder:
    """Stands in for the native library: records every call, returns success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, *args))
            return 0

        return call


@pytest.fixture
def applied(monkeypatch):
    from nos_amd import ops

    rec = _Recorder()
    monkeypatch.setattr(ops._lib, "lib", lambda: rec)
    # the three settings kept in Python
    for name in ("_F32_MATH", "_LN_HANDOFF", "_ATTN_F32_VARIANT"):
        monkeypatch.setattr(ops, name, getattr(ops, name))

    def apply(cfg):
        del rec.calls[:]
        ops.apply_kernel_config(cfg)
        return sorted(rec.calls), (ops.f32_math(), ops._LN_HANDOFF, ops.attention_f32_variant())

    return apply


# every native setter once, with the codes of the named values (ops.set_*)
_WHOLE = [("nos_attn_f32_set_variant", 0), ("nos_attn_f32x6_set_kvsplit", 0), ("nos_gemm_f32_set_policy", 1),
          ("nos_gemm_f32h3_set_hot_bn", 128), ("nos_gemm_f32h3_set_hot_ring", 2),
          ("nos_gemm_f32h3_set_lds_epilogue", 1), ("nos_gemm_f32x6_set_tile", -1), ("nos_gemm_set_policy", 1)]


def test_apply_kernel_config_reaches_every_setter_once(applied):
    from nos_amd.models.pod import kernel_config

    whole = kernel_config(None, {})
    assert len(whole) == 9  # the keys of tests/test_podbench.py::test_pod_kernel_config_follows_the_slice
    assert applied(whole) == (_WHOLE, ("h3", True, "h3"))
    # the 36 / 288 slice: throughput bf16 tiles, small fp32 tiles, keys never split, x6 GEMMs on 128 x 128
    frac = dict(_WHOLE, nos_gemm_set_policy=0, nos_gemm_f32_set_policy=2, nos_attn_f32x6_set_kvsplit=1,
                nos_gemm_f32x6_set_tile=5)
    assert applied(kernel_config(36 / 288, {})) == (sorted(frac.items()), ("h3", True, "h3n"))
    # every key reaches its setter: a config that differs from the defaults everywhere
    env = {"NOS_AMD_GEMM_POLICY": "wide", "NOS_AMD_GEMM_F32_POLICY": "throughput", "NOS_AMD_ATTN_F32_VARIANT": "w4k32",
           "NOS_AMD_F32_MATH": "x6", "NOS_AMD_X6_TILE": "128x64", "NOS_AMD_LN_HANDOFF": "off",
           "NOS_AMD_H3_EPILOGUE": "regs", "NOS_AMD_H3_HOT_RING": "3", "NOS_AMD_H3_HOT_BN": "64"}
    other = [("nos_attn_f32_set_variant", 3), ("nos_gemm_f32_set_policy", 0), ("nos_gemm_f32h3_set_hot_bn", 64),
             ("nos_gemm_f32h3_set_hot_ring", 3), ("nos_gemm_f32h3_set_lds_epilogue", 0),
             ("nos_gemm_f32x6_set_tile", 3), ("nos_gemm_set_policy", 4)]
    assert applied(kernel_config(None, env)) == (other, ("x6", False, "w4k32"))


def test_apply_kernel_config_defaults_of_missing_keys(applied):
    # the keys a pod server's config has always had to name; the rest as the server defaulted them
    required = {"gemm_bf16": "latency", "gemm_f32": "latency", "attention_f32": "h3", "f32_math": "h3",
                "gemm_f32x6_tile": "policy"}
    assert applied(required) == (_WHOLE, ("h3", True, "h3"))
    with pytest.raises(KeyError):
        applied({})
