"""Greedy speculative decoding of decoder tenants on the CPU: the builder's
rules, the new ops in the validator, the CPU fallbacks of ``spec_accept`` and
``spec_draft`` against literal Python, and generation on a CPU pod server
against ``transformers`` and the plain tenant -- token for token.

The contract (docs/tenant_programs.md): ``hist[b, t]`` is the token at
position t for every t <= ``pos[b]``, ``hist[b, pos[b]]`` the pending one; a
verify step takes the pending token and K - 1 drafts, accepts the drafts the
model's own draws confirm plus one more token, and advances ``pos`` by that
many -- never past the cache or the request's ``end``."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from nos_amd.models.llama_program import (dequantized_llama, kv_q8_roundtrip_cache, llama_config,
                                          llama_decode_programs, llama_model)
from nos_amd.ops import tenant as T
from nos_amd.podserver import program as PG
from nos_amd.podserver.client import PodClient, PodServerError
from nos_amd.podserver.server import PodServer

MAX_LEN, N = 256, 48
PROMPTS = ([5, 9, 17, 5, 9, 17, 5, 9], [343, 46, 12, 400, 3, 77])
MIN_GAP = 1e-4   # of max |logit|: ten times the 1e-5 the decode logits are held to (tests/test_stopping_gpu.py)
# the advances by 1 / 2 / 3 / 4 of the draft rule at K = 4 over transformers' tokens, per prompt
HISTOGRAMS = ({1: 12, 2: 6, 3: 1, 4: 5}, {1: 16, 2: 2, 3: 1, 4: 6})


# ------------------------------------------------------------------ the rule, in literal Python
def draft_rule(h: list, k: int) -> list:
    """[pending, k - 1 drafts] for the history h (its last token pending)."""
    p = len(h) - 1
    out = [h[p]] * k
    for n in (3, 2, 1):
        if p + 1 < n + 1:
            continue
        hits = [t for t in range(n - 1, p) if h[t - n + 1:t + 1] == h[p - n + 1:p + 1]]
        if hits:
            t = max(hits)
            for j in range(1, k):
                if t + j <= p:
                    out[j] = h[t + j]
            break
    return out


def accept_rule(ids: list, g: list, p: int, end: int, limit: int) -> int:
    if not 0 <= p < limit:
        return 0
    a = 0
    for j in range(1, len(ids)):
        if ids[j] != g[j - 1]:
            break
        a += 1
    m = min(a + 1, limit - 1 - p)
    if end > 0:
        m = min(m, end - p)
    return max(m, 0)


def simulate(seq: list, P: int, k: int, first=None) -> list:
    """The advances of a speculating generation whose model emits ``seq[P:]`` after the prompt
    ``seq[:P]``: ``first`` (default: the rule's) are the first step's [pending, drafts]."""
    end, p, adv = len(seq) - 1, P, []
    while p < end:
        ids = first if first is not None and not adv else draft_rule(seq[:p + 1], k)
        a = 0
        while a + 1 < k and p + a + 1 <= end and ids[a + 1] == seq[p + a + 1]:
            a += 1
        m = min(a + 1, end - p)
        adv.append(m)
        p += m
    return adv


# ------------------------------------------------------------------ CPU fallbacks
def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def test_speculate_ctl():
    assert T.speculate_ctl(55).tolist() == [55, 0, 0, 0] and T.speculate_ctl().tolist() == [0, 0, 0, 0]
    for bad in (-1, 1.5, True, 1 << 31):
        with pytest.raises(ValueError, match="end"):
            T.speculate_ctl(bad)


@pytest.mark.parametrize("K", [2, 4, 8])
def test_spec_accept_fallback_is_the_literal_loop(K):
    L = 32
    rows = []   # (ids, g, p, end)
    pend, drafts = 7, list(range(100, 100 + K - 1))
    for a in range(K):   # the first a drafts confirmed, then a mismatch
        g = drafts[:a] + [999] * (K - a)
        rows += [([pend] + drafts, g, 5, 0), ([pend] + drafts, g, 5, 5 + a), ([pend] + drafts, g, 5, 5),
                 ([pend] + drafts, g, L - 2, 0), ([pend] + drafts, g, L - 1, 0), ([pend] + drafts, g, L - 2, L + 9)]
    if K > 2:   # a re-match after a mismatch does not count
        rows.append(([pend] + drafts, [999] + drafts[1:] + [5], 5, 0))
    rows += [([pend] + drafts, drafts + [1], -1, 0), ([pend] + drafts, drafts + [1], L, 0),
             ([pend] + drafts, drafts + [1], 9, 4)]   # counters outside [0, L); end behind the counter
    for ids, g, p, end in rows:
        got = T.spec_accept(_i32([ids]), _i32([g]), _i32([p]), torch.from_numpy(T.speculate_ctl(end)), L)
        assert got.tolist() == [accept_rule(ids, g, p, end, L)], (ids, g, p, end)
    # known values: all confirmed, none, the cache's last rows, the budget, a hold
    full = lambda p, end: int(T.spec_accept(_i32([[pend] + drafts]), _i32([drafts + [1]]), _i32([p]),  # noqa: E731
                                            torch.from_numpy(T.speculate_ctl(end)), L)[0])
    assert [full(5, 0), full(L - 2, 0), full(L - 1, 0), full(5, 6), full(5, 5), full(-1, 0), full(L, 0)] == \
        [K, 1, 0, 1, 0, 0, 0]
    # rows are independent
    ids = _i32([r[0] for r in rows])
    got = T.spec_accept(ids, _i32([r[1] for r in rows]), _i32([r[2] for r in rows]),
                        torch.from_numpy(T.speculate_ctl(0)), L)
    assert got.tolist() == [accept_rule(r[0], r[1], r[2], 0, L) for r in rows]


def test_spec_draft_fallback():
    cases = {
        "3-gram, the more recent of two": ([1, 2, 3, 40, 1, 2, 3, 50, 60, 1, 2, 3], 4, [3, 50, 60, 1]),
        "only a 1-gram": ([4, 5, 6, 9, 8, 6], 4, [6, 9, 8, 6]),
        "no match": ([4, 5, 6, 7], 4, [7, 7, 7, 7]),
        "continuation past p'": ([8, 9, 8, 9], 8, [9, 8, 9, 9, 9, 9, 9, 9]),
        "2-gram beats a later 1-gram": ([1, 2, 30, 2, 40, 1, 2], 3, [2, 30, 2]),
        "p' = 0": ([3], 4, [3, 3, 3, 3]),
        "p' = 1, a 1-gram": ([3, 3], 2, [3, 3]),
    }
    for name, (h, k, want) in cases.items():
        hist = torch.full((1, 16), -7, dtype=torch.int32)
        hist[0, :len(h)] = _i32(h)
        got = T.spec_draft(hist, _i32([len(h) - 1]), k)[0].tolist()
        assert got == want == draft_rule(h, k), (name, got)
    rng = np.random.default_rng(0)   # a small alphabet: matches of every length
    for _ in range(200):
        L = int(rng.integers(1, 40))
        h = rng.integers(0, 3, L).tolist()
        hist = torch.zeros((2, 48), dtype=torch.int32)
        hist[1, :L] = _i32(h)
        got = T.spec_draft(hist, _i32([48, L - 1]), 5)
        assert got[1].tolist() == draft_rule(h, 5) and got[0].tolist() == [0] * 5   # a counter past the row: zeros


def test_spec_step_fallback_and_hist_write():
    L, K = 16, 4
    hist = torch.zeros((3, L), dtype=torch.int32)
    hist[0, :6] = _i32([1, 2, 3, 1, 2, 77])          # 77 is stale: the step writes the pending id there
    hist[1, :4] = _i32([5, 5, 5, 5])
    hist[2] = 9
    pos = _i32([5, 3, L])
    before = hist.clone()
    ids, g = _i32([[3, 1, 2, 3], [5, 6, 6, 6], [1, 1, 1, 1]]), _i32([[1, 2, 8, 9], [5, 5, 5, 5], [1, 1, 1, 1]])
    nxt, m = T.spec_step(hist, pos, ids, g, torch.from_numpy(T.speculate_ctl(0)))
    assert m.tolist() == [3, 1, 0] and pos.tolist() == [8, 4, L]
    assert hist[0, :9].tolist() == [1, 2, 3, 1, 2, 3, 1, 2, 8] and hist[1, :5].tolist() == [5, 5, 5, 5, 5]
    assert torch.equal(hist[2], before[2]) and torch.equal(hist[0, 9:], before[0, 9:])
    assert nxt.tolist() == [[8, 8, 8, 8], [5, 5, 5, 5], [0, 0, 0, 0]]
    # a hold (end == p): nothing changes, the next input is the row's own pending token and drafts
    hold = hist.clone()
    nxt2, m2 = T.spec_step(hist, pos, nxt, g, torch.from_numpy(T.speculate_ctl(4)))
    assert m2.tolist() == [0, 0, 0] and torch.equal(hist, hold) and pos.tolist() == [8, 4, L]
    assert nxt2[1].tolist() == [5, 5, 5, 5]
    # hist_write: ids then tail from pos - back on, indices outside the row dropped
    h = torch.zeros((2, 6), dtype=torch.int32)
    T.hist_write(h, _i32([3, 6]), _i32([[1, 2, 3], [4, 5, 6]]), _i32([[7], [8]]), back=3)
    assert h.tolist() == [[1, 2, 3, 7, 0, 0], [0, 0, 0, 4, 5, 6]]
    T.hist_write(h, _i32([-1, 4]), _i32([[9, 9], [9, 9]]))
    assert h.tolist() == [[9, 2, 3, 7, 0, 0], [0, 0, 0, 4, 9, 9]]


# ------------------------------------------------------------------ builder and validator
@pytest.fixture(scope="module")
def model():
    return llama_model(llama_config(False), 0)


def test_builder_refusals(model):
    mk = lambda **kw: llama_decode_programs(model, 6, MAX_LEN, **kw)  # noqa: E731
    for kw, msg in (({"speculate": 1}, r"speculate must be an int in \[2, 8\]"),
                    ({"speculate": 9}, r"speculate must be an int in \[2, 8\]"),
                    ({"speculate": True}, r"speculate must be an int in \[2, 8\]"),
                    ({"speculate": 4, "batch": 3}, r"batch \* K = 12 > 8 \(GEMV_MAX_ROWS\)"),
                    ({"speculate": 8, "batch": 2}, r"batch \* K = 16 > 8"),
                    ({"speculate": 4, "dtype": "bf16"}, r"dtype must be 'fp32'"),
                    ({"speculate": 4, "sampling": True}, r"greedy only"),
                    ({"speculate": 4, "stopping": True}, r"greedy only"),
                    ({"speculate": 4, "extend": (2, 4)}, r"K = 4 is also .* extend length"),
                    ({"speculate": 6}, r"K = 6 is also the prompt length")):
        with pytest.raises(ValueError, match=msg):
            mk(**kw)
    # int8 weights: the verify step's rows must fit the int8 GEMV's x staging (no transient fp32 weight);
    # the same tenant with fp32 weights, and a narrower step, are built
    wide = llama_model(llama_config(False, intermediate_size=4096, num_hidden_layers=1), 0)
    with pytest.raises(ValueError, match=r"8 rows of 4096 inputs are more than the int8 GEMV stages \(65536 bytes"):
        llama_decode_programs(wide, 6, MAX_LEN, speculate=8, weights="int8")
    for kw in ({"speculate": 4, "weights": "int8"}, {"speculate": 8}):
        assert len(llama_decode_programs(wide, 6, MAX_LEN, **kw)[0]) == 3
    for kw in ({"weights": "int8"}, {"kv": "int8"}, {"weights": "int8", "kv": "int8"}, {"batch": 2}, {"extend": (2,)}):
        progs, w = mk(speculate=4, **kw)
        ps = PG.parse_variants(progs, w)
        assert ps[-1].inputs[0].shape == (kw.get("batch", 1), 4)
        if kw.get("weights") == "int8":   # no transient dequantized weight: every linear stays a linear_q8 step
            c = ps[-1].compile("cpu")
            assert c.stats["q8_linears"] == sum(n.op == "linear_q8" for n in ps[-1].nodes) > 0


def test_no_change_by_default(model):
    for kw in ({}, {"batch": 2, "extend": (4,)}, {"weights": "int8", "kv": "int8"}):
        plain = llama_decode_programs(model, 6, 64, **kw)
        assert llama_decode_programs(model, 6, 64, speculate=None, **kw) == plain
        new = {"hist_write", "spec_accept", "pos_advance", "spec_draft"}
        for p in plain[0]:
            assert not new & {n["op"] for n in p["nodes"]}
            assert not {"hist", "speculate"} & {s["name"] for s in p["state"]} and p["outputs"] == ["logits", "next_ids"]


def test_speculating_programs(model):
    progs, w = llama_decode_programs(model, 6, 64, extend=(3,), speculate=4)
    plain, pw = llama_decode_programs(model, 6, 64, extend=(3,))
    assert w == pw and len(progs) == len(plain) + 1
    ps = PG.parse_variants(progs, w)
    for p in ps:
        assert (p.hist_state, p.state["hist"].shape, p.state["hist"].dtype) == ("hist", (1, 64), "i32")
        assert p.state["speculate"].shape == (4,)
    assert [p.outputs for p in ps] == [["logits", "next_ids", "spec_ids"], ["logits", "next_ids"],
                                       ["logits", "next_ids"], ["logits", "next_ids", "n_acc"]]
    assert [n.op for n in ps[1].nodes[-3:]] == ["argmax", "pos_add", "hist_write"]
    v = ps[-1]
    assert [n.op for n in v.nodes[-5:]] == ["argmax", "spec_accept", "hist_write", "pos_advance", "spec_draft"]
    assert v.speculate_state == "speculate" and ps[1].speculate_state is None
    assert [v.values[o].shape for o in v.outputs] == [(1, 4, 512), (1, 4), (1,)]
    c = v.compile("cpu")
    assert c.steps[-1].kind == "spec_step" and c.stats["spec_steps_fused"] == 1 and c.stats["spec_launches"] == 1
    # the static estimate charges hist like any i32 state
    extra = ps[0].state_bytes - PG.parse_variants(plain, pw)[0].state_bytes
    assert extra == 64 * 4 + 4 * 4
    assert ps[0].bytes_estimate - PG.parse_variants(plain, pw)[0].bytes_estimate >= extra


def _verify_prog(hist_len=16, ctl="speculate", ctl_decl=("speculate", [4], "i32"), second=None, k=4):
    b = PG.Builder("v")
    ids = b.input("ids", [2, k], "i32")
    tab = b.param("tab", np.ones((40, 16), np.float32))
    w = b.param("w", np.ones((40, 16), np.float32))
    b.state("pos", [2], "i32")
    b.state("hist", [2, hist_len], "i32")
    b.state("kc", [2, 16, 1, 16], "fp32")
    if ctl_decl:
        b.state(*ctl_decl)
    if second:
        b.state(second, [4], "i32")
    x = b.op("embedding", ids, tab)
    b.op("kv_write", "kc", b.op("reshape", x, shape=[2, k, 1, 16]), "pos")
    lg = b.op("linear", x, w)
    g = b.op("argmax", lg)
    if ctl == "node":
        ctl = b.op("argmax", b.op("reshape", lg, shape=[4, k * 20]))
    acc = b.op("spec_accept", ids, g, "pos", ctl, limit=16)
    if second:
        b.op("spec_accept", ids, g, "pos", second, limit=16)
    hv = b.op("hist_write", "hist", "pos", ids, g, acc, lead=1)
    nxt = b.op("spec_draft", hv, b.op("pos_advance", "pos", acc), k=k)
    return b.build([lg, nxt, acc])


def test_validator():
    p = PG.parse(*_verify_prog())
    assert (p.hist_state, p.speculate_state) == ("hist", "speculate")
    assert [p.values[o].shape for o in p.outputs[1:]] == [(2, 4), (2,)]
    for kw, msg in (({"hist_len": 12}, r"token history 'hist' has 12 positions, the caches have 16"),
                    ({"hist_len": 32}, r"token history 'hist' has 32 positions"),
                    ({"ctl": "node"}, r"spec_accept.*control words must be an i32 \[4\] state"),
                    ({"ctl": "pos"}, r"spec_accept.*control words must be an i32 \[4\] state"),
                    ({"ctl_decl": ("speculate", [8], "i32")}, r"control words must be an i32 \[4\] state"),
                    ({"second": "other"}, r"a program has one speculate state; 'speculate' and 'other' are two")):
        with pytest.raises(PG.ProgramError, match=msg):
            PG.parse(*_verify_prog(**kw))
    # the accept's limit is the history's length; the stale counter is dead after pos_advance
    prog, w = _verify_prog()
    next(n for n in prog["nodes"] if n["op"] == "spec_accept")["attrs"]["limit"] = 8
    with pytest.raises(PG.ProgramError, match=r"history 'hist' has 16 positions, the limit is 8"):
        PG.parse(prog, w)
    prog, w = _verify_prog()
    prog["nodes"][-1]["inputs"][1] = "pos"
    with pytest.raises(PG.ProgramError, match="state version 'pos' was updated in place"):
        PG.parse(prog, w)
    # one control state of each kind: sampling and speculation words are different states
    b = PG.Builder("two")
    ids = b.input("ids", [1, 2], "i32")
    b.state("pos", [1], "i32")
    b.state("hist", [1, 8], "i32")
    b.state("words", [4], "i32")
    lg = b.op("linear", b.op("embedding", ids, b.param("tab", np.ones((8, 32), np.float32))),
              b.param("w", np.ones((8, 32), np.float32)))
    g = b.op("argmax", lg)
    acc = b.op("spec_accept", ids, g, "pos", "words", limit=8)
    s = b.op("sample", b.op("slice", lg, dim=1, start=1, end=2), "words", "pos")
    b.op("hist_write", "hist", "pos", ids)
    with pytest.raises(PG.ProgramError, match="control states of different kinds must be different states"):
        PG.parse(*b.build([lg, acc, s]))


# ------------------------------------------------------------------ generation
def hf_tokens(m, prompts, n=N, **kw):
    """transformers' greedy continuation [B, n] and the smallest top-2 logit gap of its steps,
    relative to the step's max |logit|."""
    with torch.no_grad():
        out = m.generate(torch.tensor(prompts), max_new_tokens=n, do_sample=False, output_scores=True,
                         return_dict_in_generate=True, pad_token_id=0, **kw)
    gap = min(float(((t := s.float().topk(2, dim=-1).values)[:, 0] - t[:, 1]).min() / s.float().abs().max())
              for s in out.scores)
    return out.sequences[:, len(prompts[0]):].numpy().astype(np.int32), gap


@pytest.fixture(scope="module")
def hf(model):
    return [hf_tokens(model, [p]) for p in PROMPTS]


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


def test_the_inputs_meet_the_conditions(hf):
    """Conditions on the inputs, not on the code: the continuations are no near-ties, and the draft
    rule over transformers' tokens advances by 1, by something between and by K."""
    for prompt, (toks, gap), hist in zip(PROMPTS, hf, HISTOGRAMS):
        assert gap >= MIN_GAP, gap
        adv = simulate(prompt + toks[0].tolist(), len(prompt), 4)
        assert {m: adv.count(m) for m in (1, 2, 3, 4)} == hist and sum(adv) == N - 1
        for k in (4, 8):
            adv = simulate(prompt + toks[0].tolist(), len(prompt), k)
            assert 1 in adv and k in adv and any(1 < m < k for m in adv) and len(adv) < N - 1


def check_generation(c, prompts, K, want, prefill_len=None):
    """A speculating generate of N tokens: transformers' tokens, the counters at P + N - 1, and
    each step's advance the literal rule's over those tokens."""
    P = len(prompts[0])
    ids, t = c.generate(np.array(prompts, np.int32), N, speculate=True, prefill_len=prefill_len)
    assert ids.dtype == np.int32 and np.array_equal(ids, want), (ids.tolist(), want.tolist())
    assert t["state"] == {"pos": [P + N - 1] * len(prompts)}           # neither the control words nor hist
    acc = t["n_acc"]
    assert acc.shape == (t["steps_run"], len(prompts)) and acc.sum(0).tolist() == [N - 1] * len(prompts)
    assert t["steps_run"] < N - 1
    for b, prompt in enumerate(prompts):
        first = None if prefill_len is None else [int(want[b, 0])] * K   # after single steps: the pending id repeated
        adv = simulate(list(prompt) + want[b].tolist(), P, K, first)
        assert [m for m in acc[:, b].tolist() if m] == adv and not acc[len(adv):, b].any()
    vals = set(acc.ravel().tolist())
    assert 1 in vals and K in vals and any(1 < m < K for m in vals), sorted(vals)
    return ids, t


@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("which", [0, 1])
def test_generation_equals_transformers_and_the_plain_tenant(which, K, model, hf, server):
    prompt = PROMPTS[which]
    P = len(prompt)
    head = P - 1 if P == K else None   # a prompt as long as the verify step is wide: its last id as a decode step
    c = _client(server, llama_decode_programs(model, head or P, MAX_LEN, speculate=K), "spec")
    g = _client(server, llama_decode_programs(model, P, MAX_LEN), "plain")
    plain, _ = g.generate(np.array([prompt], np.int32), N)
    assert np.array_equal(plain, hf[which][0])
    check_generation(c, [prompt], K, plain, prefill_len=head)
    check_generation(c, [prompt], K, plain, prefill_len=head)   # a second sequence on the same tenant
    c.close()
    g.close()


def test_batch_of_two(model, server):
    prompts = [PROMPTS[0], PROMPTS[1] + PROMPTS[1][:2]]
    want, gap = hf_tokens(model, prompts)
    assert gap >= MIN_GAP, gap
    c = _client(server, llama_decode_programs(model, 8, MAX_LEN, batch=2, speculate=4), "spec2")
    _, t = check_generation(c, prompts, 4, want)
    assert any(a != b for a, b in t["n_acc"].tolist())   # the rows advance by different amounts
    c.close()


@pytest.mark.parametrize("fmt,which", [("weights", 0), ("weights", 1), ("kv", 1)])
def test_int8_formats(fmt, which, model, server):
    """Against the model each format computes.  The first prompt under int8 caches is left out: its
    continuation holds a near-tie (a top-2 gap of 1.1e-5 of max |logit| in transformers with
    ``kv_q8_roundtrip_cache()``), below what decides a token."""
    prompt = PROMPTS[which]
    if fmt == "weights":
        want, gap = hf_tokens(dequantized_llama(model), [prompt])
    else:
        want, gap = hf_tokens(model, [prompt], past_key_values=kv_q8_roundtrip_cache())
    assert gap >= MIN_GAP, gap
    c = _client(server, llama_decode_programs(model, len(prompt), MAX_LEN, speculate=4, **{fmt: "int8"}), "q8")
    check_generation(c, [prompt], 4, want)
    c.close()


def test_client_supplied_drafts(model, hf, server):
    prompt, K = PROMPTS[1], 4
    P, toks = len(prompt), hf[1][0][0].tolist()
    c = _client(server, llama_decode_programs(model, P, MAX_LEN, speculate=K), "own")
    x = np.array([prompt], np.int32)
    for j in (None, 1, 2, 3):   # the true continuation; a wrong id at column j
        outs, rep = c.infer(x, outputs=[1])
        assert outs[0].ravel().tolist() == toks[:1] and rep["state"] == {"pos": [P]}
        ids = np.array([toks[:K]], np.int32)
        if j is not None:
            ids[0, j] = (ids[0, j] + 1) % 512
        (logits, nxt, acc), rep = c.infer(ids, outputs=True)
        m = K if j is None else j
        assert logits.shape == (1, K, 512) and acc.tolist() == [m] and rep["state"] == {"pos": [P + m]}
        assert int(nxt[0, 0]) == toks[m]                       # the new pending token
        (_, nxt2, acc2), rep = c.infer(nxt.astype(np.int32), outputs=True)
        m2 = int(acc2[0])
        assert m2 >= 1 and rep["state"] == {"pos": [P + m + m2]} and int(nxt2[0, 0]) == toks[m + m2]
    c.close()


def test_single_steps_then_speculation(model, hf, server):
    prompt, K = PROMPTS[0], 4
    P = len(prompt)
    c = _client(server, llama_decode_programs(model, P, MAX_LEN, speculate=K), "mix")
    outs, _ = c.infer(np.array([prompt], np.int32), outputs=[1])
    toks = [int(outs[0].ravel()[0])]
    for _ in range(3):
        outs, rep = c.infer(np.array([[toks[-1]]], np.int32), outputs=[1])
        toks.append(int(outs[0].ravel()[0]))
    assert rep["state"] == {"pos": [P + 3]}
    rest, acc, rep = c.speculate_loop(np.full((1, K), toks[-1], np.int32), N - 4, P + N - 1)
    assert toks[:3] + rest[0].tolist() == hf[0][0][0].tolist()
    assert rep["state"] == {"pos": [P + N - 1]} and acc.sum() == N - 4 and rep["steps_run"] < N - 4
    # requests that cannot be served
    for spec, msg in (({"end": -1}, "end"), ({"stop": 3}, "speculate must be an object"), ([5], "speculate must be"),
                      ({"end": MAX_LEN}, "speculate: end"), ({"end": 2}, "speculate: end")):
        with pytest.raises(PodServerError, match=msg):
            c._call({"op": "generate", "steps": 4, "output": 1, "shape": [1, K], "dtype": "i32", "speculate": spec},
                    np.zeros((1, K), np.int32).tobytes())
    g = _client(server, llama_decode_programs(model, P, MAX_LEN), "plain")
    with pytest.raises(PodServerError, match="no verify step"):
        g._call({"op": "generate", "steps": 4, "shape": [1, 1], "dtype": "i32", "speculate": {"end": 20}},
                np.zeros((1, 1), np.int32).tobytes())
    with pytest.raises(ValueError, match="greedy only"):
        c.generate(np.array([prompt], np.int32), 8, speculate=True, temperature=0.7)
    assert np.array_equal(c.generate(np.array([prompt], np.int32), N, speculate=True)[0], hf[0][0])   # still serves
    c.close()
    g.close()
