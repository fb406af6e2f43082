"""Sampled generation (temperature, top-k, top-p, seed) on the CPU: the
reference of ``ops.tenant.sample`` -- its Philox stream, its kept set
against Hugging Face's warpers, the distribution of its draws -- the
``sample`` op in the validator, and the ``"sampling"`` request field on a
CPU pod server."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from nos_amd.models.llama_program import llama_config, llama_decode_programs, llama_model
from nos_amd.ops import tenant as T
from nos_amd.podserver import program as PG
from nos_amd.podserver.client import PodClient, PodServerError
from nos_amd.podserver.server import PodServer

MAX_LEN = 64
KP = [(0, 1.0), (50, 1.0), (0, 0.9), (50, 0.9), (1, 0.5)]


def test_philox4x32_known_answers():
    """Random123's known-answer vectors for Philox4x32-10."""
    kat = [([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
            "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{v:08x}" for v in T.philox4x32(ctr, key)) == want
    # a batch of counters against one key is the same function, row by row
    ctrs = np.array([k[0] for k in kat[:1]] * 3, dtype=np.uint32)
    ctrs[:, 0] = [0, 1, 2]
    rows = T.philox4x32(ctrs, np.array([5, 6], dtype=np.uint32))
    assert all(np.array_equal(rows[i], T.philox4x32(ctrs[i], [5, 6])) for i in range(3)) and len({*map(bytes, rows)}) == 3


def test_sampling_ctl_packs_and_rejects():
    c = T.sampling_ctl(0.7, 50, 0.9, 7)
    assert c.dtype == np.int32 and c.shape == (4,)
    assert c[[0, 2]].view(np.float32).tolist() == [np.float32(0.7), np.float32(0.9)] and c[[1, 3]].tolist() == [50, 7]
    assert T.sampling_ctl()[[0, 1, 3]].tolist() == [0, 0, 0]
    for bad in ({"temperature": -1.0}, {"temperature": float("inf")}, {"temperature": float("nan")}, {"top_k": -1},
                {"top_p": 0.0}, {"top_p": 1.5}, {"seed": -1}, {"seed": 1 << 31}, {"seed": 1.5}, {"top_k": 2.0},
                {"temperature": "hot"}):
        with pytest.raises(ValueError):
            T.sampling_ctl(**bad)


def _hf_kept(x: np.ndarray, temp: float, k: int, p: float) -> np.ndarray:
    """The tokens TopKLogitsWarper then TopPLogitsWarper leave, in fp64."""
    s = torch.from_numpy(x.astype(np.float64))[None] / temp
    try:
        from transformers.generation.logits_process import TopKLogitsWarper, TopPLogitsWarper
    except ImportError:
        s = s[0]
        if k > 0:
            s = s.masked_fill(s < torch.topk(s, k).values[-1], -np.inf)
        if p < 1:
            srt, idx = torch.sort(s, descending=False)
            drop = torch.softmax(srt, -1).cumsum(-1) <= 1 - p
            drop[-1] = False
            s = s.masked_fill(torch.zeros_like(drop).scatter(0, idx, drop), -np.inf)
        return torch.isfinite(s).numpy()
    if k > 0:
        s = TopKLogitsWarper(top_k=k)(None, s)
    if p < 1:
        s = TopPLogitsWarper(top_p=p)(None, s)
    return torch.isfinite(s[0]).numpy()


@pytest.mark.parametrize("k,p", KP)
def test_kept_set_is_hf_top_k_then_top_p(k, p):
    temp = 0.7
    x = (torch.randn(1000, generator=torch.Generator().manual_seed(11)) * 3).numpy()
    assert len(np.unique(x)) == 1000            # tie-free
    r = T.sample_row_ref(x, T.sampling_ctl(temp, k, p, 1))
    want = _hf_kept(x, float(np.float32(temp)), k, p)
    assert r["p_margin"] > 1e-9                  # no token on top-p's boundary: fp64 against fp64 decides nothing
    assert np.array_equal(r["keep"], want) and want.sum() == {(0, 1.0): 1000, (50, 1.0): 50, (1, 0.5): 1}.get((k, p), want.sum())
    assert r["keep"][r["token"]]


def _chi2_crit(dof: int, alpha: float = 1e-4) -> float:
    try:
        from scipy.stats import chi2

        return float(chi2.isf(alpha, dof))
    except ImportError:      # Wilson-Hilferty (within 1 % from 3 degrees of freedom on), z = the 1e-4 normal quantile
        return dof * (1 - 2 / (9 * dof) + 3.719016 * (2 / (9 * dof)) ** 0.5) ** 3


def chi2_of_draws(draws: np.ndarray, x: np.ndarray, keep: np.ndarray, temp: float) -> tuple[float, int]:
    """Pearson chi-square of the draws against softmax(x / temp) renormalised
    over ``keep`` (fp64), cells with expectation < 5 pooled: (chi2, dof)."""
    z = x.astype(np.float64) / temp
    pr = np.where(keep, np.exp(z - z[keep].max()), 0.0)
    pr /= pr.sum()
    exp = pr * len(draws)
    obs = np.bincount(draws, minlength=len(x)).astype(np.float64)
    small = keep & (exp < 5)
    cells_e = list(exp[keep & ~small]) + ([exp[small].sum()] if small.any() else [])
    cells_o = list(obs[keep & ~small]) + ([obs[small].sum()] if small.any() else [])
    e, o = np.array(cells_e), np.array(cells_o)
    return float(((o - e) ** 2 / e).sum()), len(e) - 1


@pytest.mark.parametrize("temp,k,p", [(0.7, 0, 1.0), (1.0, 10, 0.8)])
def test_draws_follow_the_renormalised_distribution(temp, k, p):
    rows, L = 4096, 50
    x = (torch.randn(L, generator=torch.Generator().manual_seed(5)) * 2)
    ctl = torch.from_numpy(T.sampling_ctl(temp, k, p, 1234))
    pos = torch.arange(rows, dtype=torch.int32)
    draws = T.sample(x.expand(rows, L), ctl, pos).numpy()
    assert pos.tolist() == list(range(rows))      # pos_n = 0: only read
    keep = T.sample_row_ref(x.numpy(), ctl.numpy())["keep"]
    assert keep[draws].all()
    chi2, dof = chi2_of_draws(draws, x.numpy(), keep, float(np.float32(temp)))
    assert dof >= 3 and chi2 < _chi2_crit(dof), (chi2, dof)


def test_greedy_cases_equal_argmax():
    x = torch.randn(6, 40)
    x[1, 7] = x[1, 30] = 9.0          # a tie: the first index
    x[2, 11] = float("nan")           # NaN wins
    x[3] = float("-inf")              # index 0
    x[4, 3] = float("inf")
    ref = torch.tensor([int(x[0].argmax()), 7, 11, 0, 3, int(x[5].argmax())], dtype=torch.int32)
    zeros = torch.zeros(4, dtype=torch.int32)
    assert torch.equal(T.sample(x, zeros), ref)
    assert torch.equal(T.sample(x, torch.tensor([0, 5, 0x3F000000, 9], dtype=torch.int32)), ref)   # T = 0, other words set
    hot = T.sample(x, torch.from_numpy(T.sampling_ctl(1.0, 0, 1.0, 3)))
    assert hot[2:5].tolist() == [11, 0, 3] and T.sample(x[:1], torch.from_numpy(T.sampling_ctl(1.0, 1, 1.0, 3))).tolist() == [ref[0]]
    with pytest.raises(ValueError):
        T.sample(x, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        T.sample(x, zeros, pos=torch.zeros(5, dtype=torch.int32))


# ------------------------------------------------------------------ validator
def _prog(ctl="ctl", ctl_decl=("ctl", [4], "i32"), pos_len=2, attrs=None, second=None):
    b = PG.Builder("s")
    x = b.input("x", [2, 16])
    w = b.param("w", np.ones((8, 16), np.float32))
    b.state("pos", [pos_len], "i32")
    if ctl_decl:
        b.state(*ctl_decl)
    if second:
        b.state(second, [4], "i32")
    lg = b.op("linear", x, w)
    if ctl == "node":
        ctl = b.op("argmax", b.op("reshape", lg, shape=[4, 4]))
    t = b.op("sample", lg, ctl, "pos", **(attrs or {}))
    outs = [t]
    if second:
        outs.append(b.op("sample", lg, second, "pos"))
    return b.build(outs)


def test_validator_takes_sample_with_a_control_state_only():
    prog, w = _prog()
    p = PG.parse(prog, w)
    assert p.sampling_state == "ctl" and p.values[p.outputs[0]].shape == (2,) and p.values[p.outputs[0]].dtype == "i32"
    for kw, msg in (({"ctl": "w"}, "state"), ({"ctl": "x"}, "state"), ({"ctl": "node"}, "state"),
                    ({"ctl_decl": ("ctl", [5], "i32")}, r"i32 \[4\]"), ({"ctl_decl": ("ctl", [4], "fp32")}, r"i32 \[4\]"),
                    ({"ctl_decl": ("ctl", [2, 2], "i32")}, r"i32 \[4\]"), ({"second": "ctl2"}, "one control state"),
                    ({"pos_len": 3}, "pos must be"), ({"attrs": {"dim": -1}}, "unknown attributes")):
        with pytest.raises(PG.ProgramError, match=msg):
            PG.parse(*_prog(**kw))


@pytest.fixture(scope="module")
def model():
    return llama_model(llama_config(False), 0)


@pytest.fixture(scope="module")
def tenants(model):
    return llama_decode_programs(model, 8, MAX_LEN), llama_decode_programs(model, 8, MAX_LEN, sampling=True)


def test_sampling_decoder_programs_validate_and_the_default_is_unchanged(model, tenants):
    (gp, gw), (sp, sw) = tenants
    progs = PG.parse_variants(sp, sw)
    assert [p.sampling_state for p in progs] == ["sampling"] * 2 and gw == sw
    assert all(p.nodes[-2].op == "sample" and p.nodes[-1].op == "pos_add" for p in progs)
    assert progs[1].nodes[-2].inputs[2] == "pos" and progs[0].nodes[-2].inputs[2] == progs[0].nodes[0].output
    assert all(p.sampling_state is None for p in PG.parse_variants(gp, gw))
    ep, ew = llama_decode_programs(model, 8, MAX_LEN, sampling=False)
    assert ep == gp and ew == gw


# ------------------------------------------------------------------ server and client
@pytest.fixture
def server(tmp_path):
    srv = PodServer(tmp_path / "s.sock", device="cpu", lanes=2, memory_gb=40).start()
    yield srv
    srv.stop()


def _client(server, tenant, name):
    progs, w = tenant
    c = PodClient(server.path, connect_timeout_s=5)
    c.register(name, progs[0], w, memory_limit_gb=1, variants=progs[1:])
    return c


def _prompt(seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 512, (1, 8)).astype(np.int32)


def test_sampled_generation_on_the_server(tenants, server):
    g, s = _client(server, tenants[0], "greedy"), _client(server, tenants[1], "sampled")
    p = _prompt(3)
    greedy, _ = g.generate(p, 12)
    a, ta = s.generate(p, 12)
    assert np.array_equal(a, greedy) and ta["state"] == {"pos": [8 + 11]}       # no sampling field: greedy, no ctl counter
    assert np.array_equal(s.generate(p, 12, temperature=0.0, top_k=5, seed=3)[0], greedy)
    kw = dict(temperature=0.8, top_k=20, top_p=0.95, seed=7)
    loop, tl = s.generate(p, 12, server_loop=True, **kw)
    step, ts = s.generate(p, 12, server_loop=False, **kw)
    assert np.array_equal(loop, step) and not np.array_equal(loop, greedy)
    assert tl["state"] == ts["state"] == {"pos": [8 + 11]}
    assert s.reset()["state"] == {"pos": [0]}
    assert np.array_equal(s.generate(p, 12, **kw)[0], loop)
    assert not np.array_equal(s.generate(p, 12, **{**kw, "seed": 8})[0], loop)
    assert np.array_equal(s.generate(p, 12)[0], greedy)                          # greedy again after a sampled request
    # the draws are the reference's at the positions before each advance: the prefill's at counter 0
    outs, _ = s.infer(p, outputs=True, sampling=kw)
    logits, nxt = outs[0].reshape(-1), int(outs[1].reshape(-1)[0])
    assert nxt == loop[0, 0] == T.sample_row_ref(logits, T.sampling_ctl(**kw), 0, 0)["token"]
    with pytest.raises(PodServerError, match="no sample node"):
        g.generate(p, 4, temperature=0.8)
    with pytest.raises(PodServerError, match="no sample node"):
        g._call({"op": "generate", "steps": 2, "shape": [1, 1], "dtype": "i32", "sampling": {"seed": 1}},
                np.array([[1]], np.int32).tobytes())
    for bad in ({"temperature": -1}, {"top_p": 0}, {"top_p": 1.5}, {"top_k": -1}, {"seed": 1.5}, {"seed": "x"},
                {"min_p": 0.1}):
        with pytest.raises(PodServerError, match="sampling"):
            s.infer(p, outputs=[1], sampling=bad)
    assert np.array_equal(s.generate(p, 12)[0], greedy)                          # and the tenant still serves
    g.close()
    s.close()
