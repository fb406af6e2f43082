"""Speculative decoding on the GPU: the two kernels of csrc/hip/decode.hip
(``spec_step_kernel``, ``hist_write_kernel``) against the CPU fallbacks of
``ops.tenant`` bit for bit, the compiled verify program of the tiny tenant
against the eager CPU reference, and generation on the GPU pod server (HIP
graphs) against the plain tenant on the same server and ``transformers`` on
the CPU.

Shapes: histories of 8 words (fewer than the workgroup's 256 threads), 300
(no multiple of it) and 8192 (the long cache: 32 candidates a thread); 1 and 3
rows; verify steps of 2, 4 and 8 tokens."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402
from nos_amd.ops import tenant as T  # noqa: E402

MAX_LEN, N = 256, 48
PROMPTS = ([5, 9, 17, 5, 9, 17, 5, 9], [343, 46, 12, 400, 3, 77])
MIN_GAP = 1e-4   # of max |logit|: ten times the 1e-5 the decode logits are held to (test_decode_step_logits_match_fp64)


@pytest.fixture(autouse=True)
def _h3():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)


# ------------------------------------------------------------------ the kernels
def _rows(K: int, L: int) -> list:
    """Rows (history, pos, ids, drawn ids, end) for a verify step of K tokens over L positions:
    every accept and draft case, each history its own."""
    rng = np.random.default_rng(1000 * K + L)
    rows = []

    def row(h, p, ids, g, end=0):
        full = rng.integers(600, 700, L)              # what lies past the counter: stale, never a match
        n = min(len(h), L)
        full[:n] = h[:n]
        rows.append((full, p, list(ids), list(g), end))

    def drafts(p):
        return rng.integers(0, 4, K - 1).tolist()

    # a small alphabet at random counters: n-gram matches of every length, continuations that run past p'
    for p in sorted({0, 1, 2, 3, L // 2, L - 4, L - 3} & set(range(L))) + rng.integers(0, L, 6).tolist():
        d = drafts(p)
        for a in range(K):                            # the first a drafts confirmed, then a mismatch
            h = rng.integers(0, 4, L)
            g = d[:a] + [9] * (K - a)
            row(h, p, [int(h[p])] + d, g)
    h = rng.integers(0, 3, L)
    d = drafts(0)
    p = min(5, L - 3)
    if K > 2:
        row(h, p, [int(h[p])] + d, [9] + d[1:] + [1])                    # a re-match after a mismatch
    full = d + [2]
    row(h, p, [int(h[p])] + d, full, end=p + 1)                          # end - p < a + 1
    row(h, p, [int(h[p])] + d, full, end=p)                              # a hold
    row(h, p, [7] + d, full, end=p)                                      # ... whatever the pending id says
    row(h, p, [int(h[p])] + d, full, end=max(p - 2, 1))                  # end behind the counter
    row(h, L - 2, [int(h[L - 2])] + d, full)                             # the cache's last rows
    row(h, L - 1, [int(h[L - 1])] + d, full)
    row(h, L - 2, [int(h[L - 2])] + d, full, end=L + 5)
    row(h, -1, [1] + d, full)                                            # counters outside [0, L): untouched
    row(h, L, [1] + d, full)
    row(h, L + 7, [1] + d, full)
    row(h, -(1 << 30), [1] + d, full)
    # the lookup's cases, by construction (a hold, so that p' = p): a 3-gram at the more recent of two
    # occurrences, only a 1-gram, no match, a continuation past p', p' = 0
    if L >= 16:
        row([1, 2, 3, 40, 1, 2, 3, 50, 60, 1, 2, 3], 11, [3] + d, full, end=11)
        row([4, 5, 6, 9, 8, 6], 5, [6] + d, full, end=5)
        row([40, 50, 60, 70], 3, [70] + d, full, end=3)
    row([8, 9, 8, 9], 3, [9] + d, full, end=3)
    row([3], 0, [3] + d, full)
    # the same n-gram far apart: candidates of the first and the last threads' strides
    if L >= 300:
        far = rng.integers(100, 200, L)
        far[0:3], far[L - 10:L - 7] = [1, 2, 3], [1, 2, 3]
        far[3] = 77
        row(far, L - 8, [3] + d, full, end=L - 8)
    return rows


@pytest.mark.parametrize("L", [8, 300, 8192])
@pytest.mark.parametrize("K", [2, 4, 8])
@pytest.mark.parametrize("B", [1, 3])
def test_spec_step_kernel_is_the_cpu_fallback(B, K, L):
    rows = _rows(K, L)
    rows += rows[:(-len(rows)) % B]
    seen = set()
    for i in range(0, len(rows), B):
        batch = rows[i:i + B]
        for end in sorted({r[4] for r in batch}):     # one control state a launch: the rows of one end together
            part = [r for r in batch if r[4] == end]
            hist = torch.from_numpy(np.stack([r[0] for r in part]).astype(np.int32))
            pos = torch.tensor([r[1] for r in part], dtype=torch.int32)
            ids = torch.tensor([r[2] for r in part], dtype=torch.int32)
            g = torch.tensor([r[3] for r in part], dtype=torch.int32)
            ctl = torch.from_numpy(T.speculate_ctl(end))
            dh, dp = hist.cuda(), pos.cuda()
            nxt, m = T.spec_step(dh, dp, ids.cuda(), g.cuda(), ctl.cuda())
            rn, rm = T.spec_step(hist, pos, ids, g, ctl)
            assert torch.equal(m.cpu(), rm) and torch.equal(dp.cpu(), pos), (part, m.tolist(), rm.tolist())
            assert torch.equal(dh.cpu(), hist) and torch.equal(nxt.cpu(), rn), (part, nxt.tolist(), rn.tolist())
            seen.update(rm.tolist())
            for r, mm in zip(part, rm.tolist()):
                if not 0 <= r[1] < L:
                    assert mm == 0
    assert seen >= set(range(0, min(K, L - 2) + 1)), seen   # every advance from a hold to K was among the cases


def test_unfused_ops_are_the_cpu_fallbacks():
    """``spec_accept``, ``pos_advance``, ``spec_draft`` and ``hist_write`` one by one (what a program
    compiled without the fusing pass launches) and together: the fused step."""
    K, L = 4, 300
    rows = _rows(K, L)
    rows = [r for r in rows if r[4] == 0]             # counters outside the row among them
    hist = torch.from_numpy(np.stack([r[0] for r in rows]).astype(np.int32))
    pos = torch.tensor([r[1] for r in rows], dtype=torch.int32)
    ids = torch.tensor([r[2] for r in rows], dtype=torch.int32)
    g = torch.tensor([r[3] for r in rows], dtype=torch.int32)
    ctl = torch.from_numpy(T.speculate_ctl(0))
    m = T.spec_accept(ids, g, pos, ctl, L)
    dm = T.spec_accept(ids.cuda(), g.cuda(), pos.cuda(), ctl.cuda(), L)
    assert torch.equal(dm.cpu(), m) and m.max() == K and m.min() == 0
    dh, dp = hist.cuda(), pos.cuda()
    fh, fp = hist.cuda(), pos.cuda()
    fused, fm = T.spec_step(fh, fp, ids.cuda(), g.cuda(), ctl.cuda())
    T.hist_write(dh, dp, ids.cuda(), g.cuda(), dm, lead=1)
    T.hist_write(hist, pos, ids, g, m, lead=1)
    assert torch.equal(dh.cpu(), hist) and torch.equal(fh, dh)
    T.pos_advance(dp, dm)
    T.pos_advance(pos, m)
    assert torch.equal(dp.cpu(), pos) and torch.equal(fp, dp) and torch.equal(fm, dm)
    dn = T.spec_draft(dh, dp, K)
    assert torch.equal(dn.cpu(), T.spec_draft(hist, pos, K)) and torch.equal(fused, dn)
    # hist_write as the decode steps use it: ids, then the drawn id, from pos - back on; strided ids;
    # more columns than threads; indices before and past the row dropped
    for B, S, Lh, back in ((1, 1, 8, 1), (3, 5, 300, 5), (2, 700, 8192, 700), (2, 4, 8, 4)):
        wide = torch.randint(0, 512, (B, S + 3), dtype=torch.int32)
        x, tail = wide[:, 1:S + 1], torch.randint(0, 512, (B, 1), dtype=torch.int32)
        p = torch.tensor([Lh - 2, 2, S][:B], dtype=torch.int32)
        h = torch.randint(0, 9, (B, Lh), dtype=torch.int32)
        d = T.hist_write(h.cuda(), p.cuda(), x.cuda(), tail.cuda(), back=back)
        assert torch.equal(d.cpu(), T.hist_write(h, p, x, tail, back=back))


# ------------------------------------------------------------------ the compiled verify program
@pytest.fixture(scope="module")
def model():
    from nos_amd.models.llama_program import llama_config, llama_model

    return llama_model(llama_config(False), 0)


def hf_tokens(m, prompts, n=N, **kw):
    with torch.no_grad():
        out = m.generate(torch.tensor(prompts), max_new_tokens=n, do_sample=False, output_scores=True,
                         return_dict_in_generate=True, pad_token_id=0, **kw)
    gap = min(float(((t := s.float().topk(2, dim=-1).values)[:, 0] - t[:, 1]).min() / s.float().abs().max())
              for s in out.scores)
    return out.sequences[:, len(prompts[0]):].numpy().astype(np.int32), gap


@pytest.fixture(scope="module")
def hf(model):
    return [hf_tokens(model, [p]) for p in PROMPTS]


@pytest.mark.parametrize("kw", [{}, {"weights": "int8", "kv": "int8"}], ids=["fp32", "w8-kvq8"])
def test_compiled_verify_program_equals_the_eager_reference(model, kw):
    """Prefill and six verify steps of the tiny tenant compiled for the GPU against the eager CPU
    reference: ``next_ids``, ``n_acc``, the counters and the history are equal, every step's K logit
    rows are within the decode logit bar of the reference's (1e-5 of max |logit|, the floor of
    ``test_decode_step_logits_match_fp64``'s e <= max(4 e32, 1e-5); fp32 also against transformers
    in fp64 with that bar itself), and the verify step's close is one launch."""
    import copy

    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    K, prompt = 4, PROMPTS[0]
    P = len(prompt)
    progs, w = llama_decode_programs(model, P, MAX_LEN, extend=(3,), speculate=K, **kw)
    ps = PG.parse_variants(progs, w, gpu=True)
    params, state, derived = ps[0].tensors("cuda"), ps[0].state_tensors("cuda"), {}
    cs = [p.compile("cuda", params=params, state=state, derived=derived) for p in ps]
    ext = PG.parse_variants(*llama_decode_programs(model, P, MAX_LEN, extend=(K,), **kw), gpu=True)[2].compile("cuda")
    v = cs[-1]
    assert v.steps[-1].kind == "spec_step" and v.stats["spec_steps_fused"] == 1
    assert v.stats["spec_launches"] == 1 and v.stats["kernels"] - ext.stats["kernels"] <= 2
    if kw:   # no transient dequantized weight: every linear of the verify step stays one int8 GEMV
        assert v.stats["q8_linears"] == sum(n.op == "linear_q8" for n in ps[-1].nodes) > 0
    ref_state = {k: (t if t.dtype in (torch.int32, torch.int8) else t.float()) for k, t in ps[0].state_tensors("cpu").items()}
    x = torch.tensor([prompt], dtype=torch.int32)
    r = ps[0].reference(x, state=ref_state)
    got = cs[0](x.cuda())
    assert torch.equal(got[1].cpu(), r[1]) and torch.equal(got[2].cpu(), r[2])
    ids, seq = r[2].clone(), []
    for i in range(6):
        p0 = int(ref_state["pos"][0])
        r = ps[-1].reference(ids, state=ref_state)
        got = v(ids.cuda())
        e = float((got[0].cpu().double() - r[0].double()).abs().max() / r[0].double().abs().max())
        print(f"step {i}: logits e = {e:.3g}, n_acc = {r[2].tolist()}")
        assert e <= 1e-5, (i, e)
        assert torch.equal(got[1].cpu(), r[1]) and torch.equal(got[2].cpu(), r[2]), (i, got[1].tolist(), r[1].tolist())
        assert torch.equal(state["pos"].cpu(), ref_state["pos"]) and torch.equal(state["hist"].cpu(), ref_state["hist"])
        seq.append((p0, ids.clone(), got[0].cpu()))
        ids = r[1].clone()
    assert int(ref_state["pos"][0]) > P + 6            # some drafts were accepted
    if not kw:   # the rows of the last step against transformers in fp64 on its input: the bar itself
        p0, ids, logits = seq[-1]
        full = torch.cat([ref_state["hist"][:, :p0].long(), ids.long()], 1)
        with torch.no_grad():
            f32 = model(full).logits[:, -K:]
            r64 = copy.deepcopy(model).double()(full).logits[:, -K:]
        e = float((logits.double() - r64).abs().max() / r64.abs().max())
        e32 = float((f32.double() - r64).abs().max() / r64.abs().max())
        print(f"against fp64: e = {e:.3g}, e32 = {e32:.3g}")
        assert e <= max(4 * e32, 1e-5), (e, e32)


# ------------------------------------------------------------------ the GPU pod server
@pytest.fixture(scope="module")
def gpu_server(tmp_path_factory):
    from nos_amd.podserver.server import PodServer

    srv = PodServer(tmp_path_factory.mktemp("spec") / "g.sock", device="cuda", lanes=2, memory_gb=40).start()
    yield srv
    srv.stop()


def _client(srv, tenant, name):
    from nos_amd.podserver.client import PodClient

    c = PodClient(srv.path, connect_timeout_s=60)
    rep = c.register(name, tenant[0][0], tenant[1], memory_limit_gb=4, variants=tenant[0][1:])
    return c, rep


def _check(t, P, K, B=1):
    acc = t["n_acc"]
    assert t["state"] == {"pos": [P + N - 1] * B}
    assert acc.shape == (t["steps_run"], B) and acc.sum(0).tolist() == [N - 1] * B
    vals = set(acc.ravel().tolist())
    assert 1 in vals and K in vals and any(1 < m < K for m in vals), sorted(vals)


@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("which", [0, 1])
def test_gpu_server_generation_equals_the_plain_tenant_and_transformers(which, K, model, hf, gpu_server):
    """48 tokens through ``PodClient.generate(speculate=True)`` on the GPU server (HIP graphs): the
    plain tenant's on the same server and transformers' on the CPU, whose every step's top-2 gap
    is at least MIN_GAP of its largest |logit| (1.06e-3 and 2.96e-4 on the two prompts)."""
    from nos_amd.models.llama_program import llama_decode_programs

    prompt = PROMPTS[which]
    P = len(prompt)
    want, gap = hf[which]
    assert gap >= MIN_GAP, gap
    head = P - 1 if P == K else None   # a prompt as long as the verify step is wide: its last id as a decode step
    c, _ = _client(gpu_server, llama_decode_programs(model, head or P, MAX_LEN, speculate=K), f"spec{K}")
    g, _ = _client(gpu_server, llama_decode_programs(model, P, MAX_LEN), "plain")
    x = np.array([prompt], np.int32)
    plain, _ = g.generate(x, N)
    assert np.array_equal(plain, want), (plain.tolist(), want.tolist())
    for _ in range(2):   # and a second sequence on the same tenant
        ids, t = c.generate(x, N, speculate=True, prefill_len=head)
        assert ids.dtype == np.int32 and np.array_equal(ids, plain), (ids.tolist(), plain.tolist())
        _check(t, P, K)
        assert t["steps_run"] < N - 1
    c.close()
    g.close()


def test_gpu_server_int8_weights_and_caches(model, gpu_server):
    """``weights="int8", kv="int8"`` against the plain int8 tenant on the same server and the model it
    computes on the CPU (``dequantized_llama`` run with ``kv_q8_roundtrip_cache()``), on the second
    prompt: that model's top-2 gap there is 2.1e-3 of max |logit|."""
    from nos_amd.models.llama_program import dequantized_llama, kv_q8_roundtrip_cache, llama_decode_programs

    prompt = PROMPTS[1]
    P, K = len(prompt), 4
    want, gap = hf_tokens(dequantized_llama(model), [prompt], past_key_values=kv_q8_roundtrip_cache())
    assert gap >= MIN_GAP, gap
    c, rep = _client(gpu_server, llama_decode_programs(model, P, MAX_LEN, speculate=K, weights="int8", kv="int8"), "q8s")
    g, _ = _client(gpu_server, llama_decode_programs(model, P, MAX_LEN, weights="int8", kv="int8"), "q8")
    x = np.array([prompt], np.int32)
    plain, _ = g.generate(x, N)
    ids, t = c.generate(x, N, speculate=True)
    assert np.array_equal(plain, want) and np.array_equal(ids, plain), (ids.tolist(), want.tolist())
    _check(t, P, K)
    assert t["steps_run"] < N - 1
    c.close()
    g.close()


def test_overrun_steps_change_nothing(model, hf, tmp_path):
    """A check window longer than the generation: the server runs all N - 1 steps, and those past
    the budget's end advance by 0 and leave the counters and the history as they were."""
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver.server import PodServer

    prompt, K = PROMPTS[1], 4
    P = len(prompt)
    srv = PodServer(tmp_path / "o.sock", device="cuda", lanes=1, memory_gb=40, stop_check_every=64).start()
    try:
        c, _ = _client(srv, llama_decode_programs(model, P, MAX_LEN, batch=2, speculate=K), "over")
        x = np.array([prompt, prompt[::-1]], np.int32)
        ids, t = c.generate(x, N, speculate=True)
        assert np.array_equal(ids[:1], hf[1][0]), ids.tolist()
        acc = t["n_acc"]
        assert t["steps_run"] == N - 1 and t["state"] == {"pos": [P + N - 1] * 2} and acc.sum(0).tolist() == [N - 1] * 2
        for b in range(2):   # once a row is at the end, every later step of it is a hold
            last = int(np.nonzero(acc[:, b])[0].max())
            assert last < N - 2 and not acc[last + 1:, b].any() and acc[:last + 1, b].all()
        # the history after the overrun is the tokens themselves: a window of 1 gives the same reply
        srv.stop_check_every = 1
        ids1, t1 = c.generate(x, N, speculate=True)
        assert np.array_equal(ids1, ids) and t1["steps_run"] < N - 1 and t1["state"] == t["state"]
        assert np.array_equal(t1["n_acc"], acc[:t1["steps_run"]])
        c.close()
    finally:
        srv.stop()
