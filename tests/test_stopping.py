"""Stop ids and the repetition penalty of decoder tenants on the CPU: the
control words, the stopping ops in the validator, and generation on a CPU pod
server against ``transformers``' ``generate(eos_token_id=[...],
pad_token_id=..., repetition_penalty=...)``.

The contract the programs keep (docs/tenant_programs.md): a row's counter
advances in every step it entered unfinished, the one that emits its stop id
included; the stop id itself is emitted and every later id of that row is the
pad id; a finished row's counter never changes again."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from nos_amd.models.llama_program import llama_config, llama_decode_programs, llama_model
from nos_amd.ops import tenant as T
from nos_amd.podserver import program as PG
from nos_amd.podserver.client import PodClient, PodServerError
from nos_amd.podserver.server import PodServer, _steps_until_done

PROMPT_LEN, MAX_LEN, PAD = 6, 64, 3
# the issue's two cases: eos_token_id, repetition_penalty, the counters after the generation
# and (c): row 0's stop id is drawn by the prefill while row 1 goes on, with a pad id that is no stop id
CASES = {"a": ([343, 116], 1.0, [10, 8]), "b": ([343, 46], 1.3, [10, 15]), "c": ([329, 116], 1.0, [6, 8])}


def prompt() -> np.ndarray:
    return np.random.default_rng(0).integers(0, 512, (2, PROMPT_LEN)).astype(np.int32)


def hf_generate(model, eos, penalty, max_new_tokens=24, scores=False):
    """transformers' greedy generation of the cases' prompt: the new ids [B, n] (and the
    processed scores of every step)."""
    with torch.no_grad():
        out = model.generate(torch.from_numpy(prompt()).long(), max_new_tokens=max_new_tokens, do_sample=False,
                             eos_token_id=eos, pad_token_id=PAD,
                             repetition_penalty=penalty if penalty != 1.0 else None,
                             output_scores=scores, return_dict_in_generate=scores)
    if scores:
        return out.sequences[:, PROMPT_LEN:].numpy().astype(np.int32), out.scores
    return out[:, PROMPT_LEN:].numpy().astype(np.int32)


# ------------------------------------------------------------------ control words
def test_stopping_ctl_packs_and_rejects():
    c = T.stopping_ctl([343, 46], 3, 1.3)
    assert c.dtype == np.int32 and c.shape == (8,)
    assert c[:1].view(np.float32)[0] == np.float32(1.3) and c[1:].tolist() == [3, 2, 343, 46, 0, 0, 0]
    assert T.stopping_ctl([7, 8, 9, 10])[1:].tolist() == [7, 4, 7, 8, 9, 10, 0]       # pad defaults to the first stop id
    assert T.stopping_ctl(5)[1:4].tolist() == [5, 1, 5]                               # an int is one stop id
    d = T.stopping_ctl()
    assert d[:1].view(np.float32)[0] == 1.0 and not d[1:].any()
    assert T.stopping_ctl([511], 0, id_bound=512)[3] == 511
    for bad, field in (({"stop_ids": [1, 2, 3, 4, 5]}, "stop_ids"), ({"stop_ids": [-1]}, "stop_ids"),
                       ({"stop_ids": [512], "id_bound": 512}, "stop_ids"), ({"stop_ids": [1.5]}, "stop_ids"),
                       ({"stop_ids": "x"}, "stop_ids"), ({"stop_ids": [True]}, "stop_ids"),
                       ({"pad_id": -1}, "pad_id"), ({"pad_id": 512, "id_bound": 512}, "pad_id"),
                       ({"pad_id": 1.0}, "pad_id"), ({"repetition_penalty": 0.0}, "repetition_penalty"),
                       ({"repetition_penalty": -1.0}, "repetition_penalty"),
                       ({"repetition_penalty": float("inf")}, "repetition_penalty"),
                       ({"repetition_penalty": float("nan")}, "repetition_penalty"),
                       ({"repetition_penalty": "2"}, "repetition_penalty"),
                       ({"repetition_penalty": 1e-60}, "repetition_penalty")):
        with pytest.raises(ValueError, match=field):
            T.stopping_ctl(**bad)


# ------------------------------------------------------------------ CPU semantics of the ops
def test_seen_mark_and_penalize_reference():
    seen = torch.full((2, 2), -1, dtype=torch.int32)
    ids = torch.tensor([[0, 31, 32, 32], [40, 5, 5, 99]], dtype=torch.int32)       # 99: outside the 64 bits, dropped
    T.seen_mark(seen, ids, reset=True)
    assert seen.tolist() == [[1 - (1 << 31), 1], [1 << 5, 1 << 8]]                 # token 31: word 0's sign bit
    T.seen_mark(seen, torch.tensor([[1], [5]], dtype=torch.int32))
    assert seen.tolist() == [[3 - (1 << 31), 1], [1 << 5, 1 << 8]]                 # no reset: the bits stay
    assert T.seen_bits(seen, 33)[0].nonzero().flatten().tolist() == [0, 1, 31, 32]
    x = torch.randn(2, 1, 33)
    x[0, 0, 0], x[0, 0, 31] = 2.0, -2.0
    for p in (1.3, 0.5):
        ctl = torch.from_numpy(T.stopping_ctl(repetition_penalty=p))
        y = T.penalize(x, seen[:, :2], ctl)
        m = T.seen_bits(seen, 33).view(2, 1, 33)
        pf = torch.tensor(p, dtype=torch.float32)
        assert torch.equal(y, torch.where(m, torch.where(x < 0, x * pf, x / pf), x)) and not torch.equal(y, x)
    for ctl in (torch.zeros(8, dtype=torch.int32), torch.from_numpy(T.stopping_ctl())):
        assert torch.equal(T.penalize(x, seen, ctl), x)


def test_stop_step_reference():
    ctl = torch.from_numpy(T.stopping_ctl([7, 9, 11], 9))
    nxt = torch.tensor([[5], [9], [6], [5]], dtype=torch.int32)
    pos, done = torch.tensor([4, 4, 4, 4], dtype=torch.int32), torch.tensor([1, 0, 0, 2], dtype=torch.int32)
    ids = T.stop_step(nxt, pos, done, ctl, n=1)
    assert ids.tolist() == [[9], [9], [6], [9]] and pos.tolist() == [4, 5, 5, 4] and done.tolist() == [1, 1, 0, 3]
    # the three ops one by one are the fused step
    pos2, done2 = torch.tensor([4, 4, 4, 4], dtype=torch.int32), torch.tensor([1, 0, 0, 2], dtype=torch.int32)
    T.stop_step(None, pos2, done2, None, n=1, mode=2)
    ids2 = T.stop_ids(nxt, done2, ctl)
    T.done_mark(done2, ids2, ctl)
    assert torch.equal(ids2, ids) and pos2.tolist() == [4, 5, 5, 4] and [bool(v) for v in done2] == [True, True, False, True]
    z = torch.zeros(8, dtype=torch.int32)
    done3 = torch.zeros(4, dtype=torch.int32)
    assert torch.equal(T.stop_step(nxt, pos, done3, z), nxt) and not done3.any()     # n_stop = 0 never sets done


# ------------------------------------------------------------------ validator
def _prog(ctl="stopping", ctl_decl=("stopping", [8], "i32"), seen_words=2, stale=False, done_len=2):
    b = PG.Builder("s")
    ids = b.input("ids", [2, 4], "i32")
    tab = b.param("tab", np.ones((40, 16), np.float32))
    w = b.param("w", np.ones((40, 16), np.float32))
    b.state("pos", [2], "i32")
    b.state("done", [done_len], "i32")
    b.state("seen", [2, seen_words], "i32")
    if ctl_decl:
        b.state(*ctl_decl)
    h = b.op("slice", b.op("embedding", ids, tab), dim=1, start=3, end=4)
    lg = b.op("linear", h, w)                                                    # [2, 1, 40]
    if ctl == "node":
        ctl = b.op("argmax", b.op("reshape", lg, shape=[8, 10]))
    pen = b.op("penalize", lg, b.op("seen_mark", "seen", ids), ctl)
    raw = b.op("argmax", pen)
    b.op("pos_add", "pos", "done", n=1)
    nxt = b.op("stop_ids", raw, "done", ctl)
    d2 = b.op("done_mark", "done", nxt, ctl)
    outs = [lg, nxt]
    if stale:
        outs.append(b.op("stop_ids", raw, "done", ctl))                          # "done" is dead after done_mark
    del d2
    return b.build(outs)


def test_validator_takes_the_stopping_ops_with_their_states_only():
    p = PG.parse(*_prog())
    assert (p.stopping_state, p.done_state, p.seen_state) == ("stopping", "done", "seen")
    assert p.values[p.outputs[1]].shape == (2, 1) and p.values[p.outputs[1]].dtype == "i32"
    for kw, msg in (({"ctl": "node"}, r"penalize.*control words must be an i32 \[8\] state"),
                    ({"ctl": "pos"}, r"penalize.*control words must be an i32 \[8\] state"),
                    ({"ctl_decl": ("stopping", [4], "i32")}, r"control words must be an i32 \[8\] state"),
                    ({"ctl_decl": ("stopping", [8], "fp32")}, r"control words must be an i32 \[8\] state"),
                    ({"seen_words": 1}, r"penalize.*seen must be an i32 \[2, 2\] bitmap"),
                    ({"seen_words": 3}, r"penalize.*seen must be an i32 \[2, 2\] bitmap"),
                    ({"done_len": 3}, r"done must be an i32 \[2\]"),
                    ({"stale": True}, r"state version 'done' was updated in place")):
        with pytest.raises(PG.ProgramError, match=msg):
            PG.parse(*_prog(**kw))
    # stop_ids and done_mark name the control words too: another state in their place is rejected by name
    for op in ("stop_ids", "done_mark"):
        prog, w = _prog()
        for n in prog["nodes"]:
            if n["op"] == op:
                n["inputs"][2] = "done"
        with pytest.raises(PG.ProgramError, match=rf"\({op}\).*control words must be an i32 \[8\] state"):
            PG.parse(prog, w)
    # pos_add's mask is the program's done state: other flags, or a value that is no state, are refused
    for mask, msg in (("other", r"\(stop_ids\): a program has one done state; 'other' and 'done' are two"),
                      ("%flags", r"\(pos_add\): done must be a state")):
        prog, w = _prog()
        prog["state"].append({"name": "other", "shape": [2], "dtype": "i32"})
        k = next(i for i, n in enumerate(prog["nodes"]) if n["op"] == "pos_add")
        prog["nodes"][k]["inputs"][1] = mask
        pen = prog["nodes"][k - 1]["inputs"][0]                                   # the argmax before it reads [2, 1, 40]
        prog["nodes"][k:k] = [{"op": "reshape", "inputs": [pen], "output": "%rows", "attrs": {"shape": [2, 40]}},
                              {"op": "argmax", "inputs": ["%rows"], "output": "%flags"}]   # an i32 [2] that is no state
        with pytest.raises(PG.ProgramError, match=msg):
            PG.parse(prog, w)


@pytest.fixture(scope="module")
def model():
    return llama_model(llama_config(False), 0)


def test_default_programs_hold_none_of_it_and_stopping_ones_validate(model):
    progs, w = llama_decode_programs(model, 8, 64)
    new = {"seen_mark", "penalize", "stop_ids", "done_mark"}
    for p in progs:
        assert not new & {n["op"] for n in p["nodes"]} and all(len(n["inputs"]) == 1 for n in p["nodes"] if n["op"] == "pos_add")
        assert {s["name"] for s in p["state"]} == {"pos", *(f"{c}c{i}" for c in "kv" for i in range(2))}
    assert llama_decode_programs(model, 8, 64, stopping=False) == (progs, w)
    sp, sw = llama_decode_programs(model, 8, 64, stopping=True, sampling=True)
    ps = PG.parse_variants(sp, sw)
    assert sw == w and all((p.stopping_state, p.done_state, p.seen_state, p.sampling_state) ==
                           ("stopping", "done", "seen", "sampling") for p in ps)
    assert [n.op for n in ps[1].nodes[-6:]] == ["seen_mark", "penalize", "sample", "pos_add", "stop_ids", "done_mark"]
    assert ps[0].state["seen"].shape == (1, 16) and ps[0].state["stopping"].shape == (8,)
    assert [n.op for n in ps[0].nodes[:2]] == ["pos_set", "embedding"] and ps[0].nodes[-7].op == "pos_set"
    assert ps[0].nodes[-6].attrs == {"reset": True} and not ps[1].nodes[-6].attrs.get("reset")
    c = ps[1].compile("cpu")
    assert [s.kind for s in c.steps[-4:]] == ["seen_mark", "penalize", "sample", "stop_step"]
    assert c.stats["stop_launches"] == 3 and c.stats["stop_steps_fused"] == 1


# ------------------------------------------------------------------ server and client
@pytest.fixture(scope="module")
def tenants(model):
    mk = lambda **kw: llama_decode_programs(model, PROMPT_LEN, MAX_LEN, batch=2, **kw)  # noqa: E731
    return {"plain": mk(), "stop": mk(stopping=True), "plain_s": mk(sampling=True),
            "stop_s": mk(stopping=True, sampling=True)}


@pytest.fixture(scope="module")
def hf(model):
    return {k: hf_generate(model, eos, pen) for k, (eos, pen, _) in CASES.items()}


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


def test_trimming_counts_rows_finished_before_the_loop():
    """The loop's ids are trimmed to the first step after which every row was done.  A row the
    prefill finished emits only pad ids in the loop, and the pad id need be no stop id: its
    ``done`` flag from before the loop's first step counts, not its tokens."""
    toks = np.full((6, 2, 1), PAD, dtype=np.float32)          # as the server fetches them: [steps, B, 1]
    toks[:3, 1, 0] = [25, 153, 46]                            # row 1 stops at step 2, then pads; row 0 pads only
    assert _steps_until_done(toks, [343, 46]) == 6            # nothing known of row 0: every step
    assert _steps_until_done(toks, [343, 46], np.array([0, 0])) == 6
    assert _steps_until_done(toks, [343, 46], np.array([1, 0])) == 3
    assert _steps_until_done(toks, [343, 46], np.array([7, 1])) == 1      # all done before: one step, never none
    assert _steps_until_done(toks, [46, PAD], np.array([0, 0])) == 3      # a pad id that is a stop id is a hit
    assert _steps_until_done(toks[:2], [343, 46], np.array([1, 0])) == 2  # row 1 not done yet: all the steps


@pytest.mark.parametrize("case", sorted(CASES))
def test_generation_equals_transformers(case, tenants, hf, server):
    eos, pen, pos = CASES[case]
    c = _client(server, tenants["stop"], "stop")
    kw = dict(eos_token_id=eos, pad_token_id=PAD, repetition_penalty=pen)
    for loop in (True, False):
        ids, t = c.generate(prompt(), 24, server_loop=loop, **kw)
        assert ids.dtype == np.int32 and np.array_equal(ids, hf[case]), (loop, ids.tolist())
        assert t["state"] == {"pos": pos, "done": [1, 1]}          # neither the control words nor the bitmap
        assert t["steps_run"] == hf[case].shape[1] - 1
    if case == "b":   # the penalty changes tokens: the plain run's row 0 repeats 343 from step 6
        plain, _ = c.generate(prompt(), 24)
        assert plain[0, 6:].tolist() == [343] * 18 and not np.array_equal(plain[:, :10], hf[case])
    c.close()


def test_sampling_with_stops(tenants, server):
    c = _client(server, tenants["stop_s"], "stop-s")
    kw = dict(temperature=0.9, top_k=40, top_p=0.95, seed=11)
    free, _ = c.generate(prompt(), 24, **kw)                       # the same seeded run without stops
    stops = [int(free[0, 4]), int(free[1, 9])]
    cut = [int(np.isin(r, stops).argmax()) for r in free]          # each row's first stop id
    assert max(cut) < 23 and cut[0] != cut[1]
    want = np.full((2, max(cut) + 1), PAD, dtype=np.int32)
    for r in range(2):
        want[r, :cut[r] + 1] = free[r, :cut[r] + 1]
    for loop in (True, False):
        ids, t = c.generate(prompt(), 24, server_loop=loop, eos_token_id=stops, pad_token_id=PAD, **kw)
        assert np.array_equal(ids, want), (loop, ids.tolist(), want.tolist())
        assert t["state"] == {"pos": [PROMPT_LEN + n for n in cut], "done": [1, 1]}
    c.close()


def test_early_exit(model, tmp_path):
    eos, pen, pos = CASES["b"]
    srv = PodServer(tmp_path / "e.sock", device="cpu", lanes=1, memory_gb=40, stop_check_every=4).start()
    try:
        c = _client(srv, llama_decode_programs(model, PROMPT_LEN, 256, batch=2, stopping=True), "early")
        ids, t = c.generate(prompt(), 200, eos_token_id=eos, pad_token_id=PAD, repetition_penalty=pen)
        assert ids.shape == (2, 10) and np.array_equal(ids, hf_generate(model, eos, pen, 200))
        assert t["steps_run"] <= 9 + 2 * srv.stop_check_every and t["state"] == {"pos": pos, "done": [1, 1]}
        c.close()
    finally:
        srv.stop()
    with pytest.raises(ValueError, match="stop_check_every"):
        PodServer(tmp_path / "x.sock", device="cpu", stop_check_every=0)


def test_prefill_stop_no_field_and_rejections(tenants, hf, server):
    s, g = _client(server, tenants["stop"], "stop"), _client(server, tenants["plain"], "plain")
    plain, _ = g.generate(prompt(), 12)
    # a stop id drawn by the prefill (each row's first token) ends the generation with n == 1
    for loop in (True, False):
        ids, t = s.generate(prompt(), 12, server_loop=loop, eos_token_id=[int(plain[0, 0]), int(plain[1, 0])])
        assert ids.tolist() == plain[:, :1].tolist() and t["steps_run"] == 0
        assert t["state"] == {"pos": [PROMPT_LEN] * 2, "done": [1, 1]}
    # no stopping field: the plain tenant's tokens, every step run, whatever the request before set
    for loop in (True, False):
        ids, t = s.generate(prompt(), 12, server_loop=loop)
        assert np.array_equal(ids, plain) and t["state"] == {"pos": [PROMPT_LEN + 11] * 2, "done": [0, 0]}
        assert t["steps_run"] == 11
    # a finished row's counter stands still while the other row goes on (only row 1 ever stops)
    ids, t = s.generate(prompt(), 8, eos_token_id=116, pad_token_id=PAD)
    assert ids[1].tolist() == [25, 153, 116] + [PAD] * 5 and np.array_equal(ids[0], plain[0, :8])
    assert t["state"] == {"pos": [PROMPT_LEN + 7, PROMPT_LEN + 2], "done": [0, 1]}
    for bad, field in (({"stop_ids": [1, 2, 3, 4, 5]}, "stop_ids"), ({"stop_ids": [512]}, "stop_ids"),
                       ({"stop_ids": [-1]}, "stop_ids"), ({"pad_id": 512}, "pad_id"),
                       ({"repetition_penalty": 0}, "repetition_penalty"),
                       ({"repetition_penalty": -2.0}, "repetition_penalty"), ([343], "stopping must be an object"),
                       ("x", "stopping must be an object"), ({"eos": 3}, "stopping must be an object")):
        with pytest.raises(PodServerError, match=field):
            s._call({"op": "infer", "outputs": [1], "shape": [2, PROMPT_LEN], "dtype": "i32", "stopping": bad},
                    prompt().tobytes())
    with pytest.raises(PodServerError, match="repetition_penalty"):
        s._call({"op": "generate", "steps": 2, "shape": [2, 1], "dtype": "i32",
                 "stopping": {"repetition_penalty": float("inf")}}, np.zeros((2, 1), np.int32).tobytes())
    for call in (lambda: g.generate(prompt(), 4, eos_token_id=343),
                 lambda: g._call({"op": "generate", "steps": 2, "shape": [2, 1], "dtype": "i32",
                                  "stopping": {"stop_ids": [1]}}, np.zeros((2, 1), np.int32).tobytes())):
        with pytest.raises(PodServerError, match="stopping: the tenant's programs have no stopping state"):
            call()
    assert np.array_equal(s.generate(prompt(), 12)[0], plain)      # and the tenant still serves
    s.close()
    g.close()
