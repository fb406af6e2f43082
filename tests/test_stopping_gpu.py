"""Stop ids and the repetition penalty on the GPU: the three kernels of
csrc/hip/decode.hip (``seen_mark_kernel``, ``penalize_kernel``,
``stop_step_kernel``) against the CPU fallbacks of ``ops.tenant``, the
compiled tiny stopping programs against the eager CPU reference, and
generation on the GPU pod server (HIP graphs) against ``transformers`` on the
CPU.

Shapes: vocab 33 (two bitmap words, one of them a single bit; the scalar
path of ``penalize``), 512 (the tiny model's) and 32000 (the fleet
decoder's: several workgroups per row, the last one partly past the row);
token ids 0, 31 (a word's sign bit), 32 and vocab - 1 (the word borders)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402
from nos_amd.ops import tenant as T  # noqa: E402

PROMPT_LEN, MAX_LEN, PAD = 6, 256, 3
# (a), (b): the issue's; (c): row 0's stop id is drawn by the prefill while row 1 goes on, and the pad id is no
# stop id -- row 0 emits only pad ids in the server's loop, whose overrun steps must still be trimmed
CASES = {"a": ([343, 116], 1.0, [10, 8]), "b": ([343, 46], 1.3, [10, 15]), "c": ([329, 116], 1.0, [6, 8])}
MIN_GAP = 1e-4   # of max |logit|: ten times the 1e-5 the decode logits are held to (test_decode_step_logits_match_fp64)


@pytest.fixture(autouse=True)
def _h3():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)


def _ctl(*a, **kw) -> torch.Tensor:
    return torch.from_numpy(T.stopping_ctl(*a, **kw)).cuda()


# ------------------------------------------------------------------ seen_mark
def _ids(B: int, vocab: int, S: int, seed: int) -> torch.Tensor:
    """ids [B, S]: the border ids and duplicates first (S = 16), then ids of the row's own."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab, (B, S), generator=g, dtype=torch.int32)
    if S >= 8:
        ids[:, :6] = torch.tensor([0, 31, 32, vocab - 1, 0, vocab - 1], dtype=torch.int32)   # borders, duplicates
        ids[:, 6] = torch.arange(B, dtype=torch.int32) + 5                                    # one id per row: no leak
    else:
        ids[:, 0] = torch.tensor([0, 31, vocab - 1][:B] + [32] * max(0, B - 3), dtype=torch.int32)
    return ids


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("vocab", [33, 512, 32000])
@pytest.mark.parametrize("S", [1, 16])
def test_seen_mark_equals_the_cpu_fallback(B, vocab, S):
    W = -(-vocab // 32)
    ids = _ids(B, vocab, S, seed=B * 100 + S)
    # reset over bitmaps pre-filled with ones
    ref = T.seen_mark(torch.full((B, W), -1, dtype=torch.int32), ids, reset=True, vocab=vocab)
    seen = torch.full((B, W), -1, dtype=torch.int32, device="cuda")
    out = T.seen_mark(seen, ids.cuda(), reset=True, vocab=vocab)
    assert out.data_ptr() == seen.data_ptr() and torch.equal(seen.cpu(), ref)
    bits = T.seen_bits(ref, vocab)
    for r in range(B):   # exactly the row's ids: nothing leaks across rows
        assert sorted(bits[r].nonzero().flatten().tolist()) == sorted(set(ids[r].tolist()))
    # no reset: the earlier bits stay; ids outside [0, vocab) are ignored
    more = _ids(B, vocab, S, seed=7)
    more[:, -1] = torch.tensor([-1, vocab, 1 << 30][:B] + [vocab] * max(0, B - 3), dtype=torch.int32)
    ref2 = T.seen_mark(ref.clone(), more, vocab=vocab)
    T.seen_mark(seen, more.cuda(), vocab=vocab)
    assert torch.equal(seen.cpu(), ref2) and bool(((ref2 & ref) == ref).all())
    if vocab >= 96:   # all of 64 .. 95 in one call: the word reads -1, its neighbours as before
        full = torch.arange(64, 96, dtype=torch.int32).repeat(B, 1)
        ref3 = T.seen_mark(ref2.clone(), full, vocab=vocab)
        T.seen_mark(seen, full.cuda(), vocab=vocab)
        assert torch.equal(seen.cpu(), ref3) and seen[:, 2].tolist() == [-1] * B
        assert torch.equal(seen.cpu()[:, :2], ref2[:, :2]) and torch.equal(seen.cpu()[:, 3:], ref2[:, 3:])
    # a strided ids view (the last column of a wider tensor) is read through its row stride
    wide = torch.randint(0, vocab, (B, 5), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    z = torch.zeros((B, W), dtype=torch.int32, device="cuda")
    T.seen_mark(z, wide.cuda()[:, :2])
    assert torch.equal(z.cpu(), T.seen_mark(torch.zeros((B, W), dtype=torch.int32), wide[:, :2]))


# ------------------------------------------------------------------ penalize
SPECIAL = [0.0, -0.0, float("-inf"), float("inf"), float("nan"), 1e30, -1e30, 3e-30, -7.5]


def _logits(rows: int, vocab: int, seed: int):
    """(x fp32 [rows, vocab] with the special values at seen and at unseen positions, seen [rows, W])."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, vocab, generator=g) * 4
    marked = torch.rand(rows, vocab, generator=g) < 0.3
    n = len(SPECIAL)
    for r in range(rows):
        at = torch.randperm(vocab, generator=g)[:2 * n] if vocab >= 2 * n else torch.arange(2 * n) % vocab
        x[r, at] = torch.tensor(SPECIAL * 2)
        marked[r, at[:n]], marked[r, at[n:]] = True, False
    marked[:, [0, 31 % vocab, 32 % vocab, vocab - 1]] = True
    ids = [marked[r].nonzero().flatten().to(torch.int32) for r in range(rows)]
    seen = torch.zeros((rows, -(-vocab // 32)), dtype=torch.int32)
    for r in range(rows):
        T.seen_mark(seen[r:r + 1], ids[r][None], vocab=vocab)
    assert torch.equal(T.seen_bits(seen, vocab), marked)
    return x, seen, marked


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-equal (so -0 is not +0), NaN matching NaN whatever its payload."""
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a.view(it)[~nan], b.view(it)[~nan])


@pytest.mark.parametrize("p", [1.0, 1.3, 0.5])
@pytest.mark.parametrize("vocab,ld", [(33, 33), (33, 40), (512, 512), (512, 520), (512, 515), (2500, 2500),
                                      (32000, 32008)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_penalize_is_bit_equal(dtype, vocab, ld, p):
    """fp32: bit-equal to ``torch.where(x < 0, x * p, x / p)`` on the seen positions (fp32 on the
    CPU: IEEE multiply and divide, which the kernel's are -- hipcc divides correctly rounded
    unless told otherwise and the build passes no fast-math flag), an exact copy elsewhere; bf16:
    that fp32 math on the bf16 values, rounded once.  Row strides: the vocab, a larger multiple of
    four (vector loads), one that is not (scalar loads); vocab 33 and 2500 end inside a thread's
    four logits / a workgroup's 1024."""
    rows = 3 if vocab <= 512 else 2
    x, seen, marked = _logits(rows, vocab, seed=vocab + ld)
    x = x.to(dtype)
    pf = torch.tensor(p, dtype=torch.float32)
    xf = x.float()
    want = torch.where(marked, torch.where(xf < 0, xf * pf, xf / pf), xf).to(dtype)
    if p == 1.0:
        assert _same_bits(want, x)
    buf = torch.full((rows, ld), 77.0, dtype=dtype, device="cuda")
    buf[:, :vocab] = x.cuda()
    xg = buf[:, :vocab]                                             # rows at stride ld
    before = buf.clone()
    for ctl in ([_ctl(repetition_penalty=p)] + ([torch.zeros(8, dtype=torch.int32, device="cuda")] if p == 1.0 else [])):
        y = T.penalize(xg, seen.cuda(), ctl)
        assert y.shape == xg.shape and y.dtype == dtype and y.is_contiguous() and y.data_ptr() != buf.data_ptr()
        assert _same_bits(y.cpu(), want), (y.cpu().float() - want.float()).abs().nan_to_num(0).max()
        assert _same_bits(buf.cpu(), before.cpu())                  # the raw logits are only read
        assert _same_bits(T.penalize(x, seen, ctl.cpu()), want)     # and the CPU fallback is the same function
    y3 = T.penalize(xg.view(rows, 1, vocab) if ld == vocab else xg.unsqueeze(1), seen.cuda(), _ctl(repetition_penalty=p))
    assert y3.shape == (rows, 1, vocab) and _same_bits(y3.cpu().view(rows, vocab), want)


def test_penalize_rejects_bad_arguments():
    x, seen = torch.zeros(2, 64, device="cuda"), torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    ctl = _ctl()
    for args in ((x, seen[:, :1].contiguous(), ctl), (x, seen[:1], ctl), (x, seen.float(), ctl), (x, seen, ctl[:4]),
                 (x, seen, ctl.cpu()), (x, seen.cpu(), ctl), (x.double(), seen, ctl)):
        with pytest.raises(ValueError):
            T.penalize(*args)
    with pytest.raises(ValueError):
        T.seen_mark(seen, torch.zeros(3, 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        T.seen_mark(seen, torch.zeros(2, 1, dtype=torch.int32, device="cuda"), vocab=65)


# ------------------------------------------------------------------ stop_step
def test_stop_step_rows():
    """B = 4 in one call, three stop ids (7, 9, 11), pad 9 (itself a stop id): row 1 already done,
    row 2 emits stop id #2 of 3, row 3 a non-stop id, row 4 done with the pad a stop id."""
    ctl = T.stopping_ctl([7, 9, 11], 9)
    nxt = torch.tensor([[5], [9], [6], [5]], dtype=torch.int32)
    pos0, done0 = torch.tensor([4, 14, 24, 34], dtype=torch.int32), torch.tensor([1, 0, 0, 1], dtype=torch.int32)
    pos, done = pos0.cuda(), done0.cuda()
    ids = T.stop_step(nxt.cuda(), pos, done, torch.from_numpy(ctl).cuda(), n=1)
    assert ids.shape == (4, 1) and ids.flatten().tolist() == [9, 9, 6, 9]       # pad, kept, unchanged, pad
    assert pos.tolist() == [4, 15, 25, 34] and done.tolist() == [1, 1, 0, 1]   # held, advanced, advanced, held
    rp, rd = pos0.clone(), done0.clone()
    assert torch.equal(T.stop_step(nxt, rp, rd, torch.from_numpy(ctl), n=1), ids.cpu())
    assert torch.equal(rp, pos.cpu()) and torch.equal(rd, done.cpu())
    # a pad id that is no stop id leaves a finished row finished; n > 1 (an extend chunk) advances by n
    ctl2 = _ctl([7, 9, 11], 2)
    pos, done = pos0.cuda(), done0.cuda()
    assert T.stop_step(nxt.cuda(), pos, done, ctl2, n=5).flatten().tolist() == [2, 9, 6, 2]
    assert pos.tolist() == [4, 19, 29, 34] and done.tolist() == [1, 1, 0, 1]
    # the three ops one by one (their own launches) are the fused step
    pos, done = pos0.cuda(), done0.cuda()
    T.stop_step(None, pos, done, None, n=1, mode=2)
    one = T.stop_ids(nxt.cuda(), done, ctl2)
    assert T.done_mark(done, one, ctl2).data_ptr() == done.data_ptr()
    assert one.flatten().tolist() == [2, 9, 6, 2] and pos.tolist() == [4, 15, 25, 34] and done.tolist() == [1, 1, 0, 1]
    # n_stop = 0 never sets done, whatever the stop slots hold
    for words in (np.zeros(8, np.int32), np.array([0, 3, 0, 5, 6, 9, 5, 0], np.int32)):
        pos, done = pos0.cuda(), torch.zeros(4, dtype=torch.int32, device="cuda")
        assert torch.equal(T.stop_step(nxt.cuda(), pos, done, torch.from_numpy(words).cuda()).cpu(), nxt)
        assert done.tolist() == [0] * 4 and pos.tolist() == [5, 15, 25, 35]
    # 300 rows: more than one workgroup
    g = torch.Generator().manual_seed(1)
    nx, dn = torch.randint(0, 16, (300,), generator=g, dtype=torch.int32), (torch.rand(300, generator=g) < 0.3).int()
    ps = torch.arange(300, dtype=torch.int32)
    gp, gd = ps.cuda(), dn.cuda()
    gi = T.stop_step(nx.cuda(), gp, gd, ctl2, n=1)
    assert torch.equal(gi.cpu(), T.stop_step(nx, ps, dn, ctl2.cpu(), n=1)) and torch.equal(gp.cpu(), ps) and torch.equal(gd.cpu(), dn)


# ------------------------------------------------------------------ compiled programs, the pod server
@pytest.fixture(scope="module")
def model():
    from nos_amd.models.llama_program import llama_config, llama_model

    return llama_model(llama_config(False), 0)


@pytest.fixture(scope="module")
def tenant(model):
    from nos_amd.models.llama_program import llama_decode_programs

    return llama_decode_programs(model, PROMPT_LEN, MAX_LEN, batch=2, stopping=True)


def _prompt() -> np.ndarray:
    return np.random.default_rng(0).integers(0, 512, (2, PROMPT_LEN)).astype(np.int32)


def test_compiled_stopping_programs_equal_the_eager_reference(model, tenant):
    """The tiny stopping programs compiled for the GPU -- prefill and 9 steps under case (b) --
    against the eager CPU reference: ids, counters and flags; and what stopping costs a decode
    step: three launches (mark, penalise, stop step)."""
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    progs, w = tenant
    ps = PG.parse_variants(progs, w, gpu=True)
    params, state, derived = ps[0].tensors("cuda"), ps[0].state_tensors("cuda"), {}
    cs = [p.compile("cuda", params=params, state=state, derived=derived) for p in ps]
    plain = PG.parse_variants(*llama_decode_programs(model, PROMPT_LEN, MAX_LEN, batch=2), gpu=True)[1].compile("cuda")
    kinds = [s.kind for s in cs[1].steps]
    assert cs[1].stats["stop_launches"] == 3 and cs[1].stats["stop_steps_fused"] == 1
    assert cs[1].stats["kernels"] == plain.stats["kernels"] + 3 and "stop_launches" not in plain.stats
    assert kinds[-4:] == ["seen_mark", "penalize", "argmax", "stop_step"] and "pos_add" not in kinds
    eos, pen, pos = CASES["b"]
    ctl = T.stopping_ctl(eos, PAD, pen, 512)
    ref_state = {k: (t if t.dtype in (torch.int32, torch.int8) else t.float()) for k, t in ps[0].state_tensors("cpu").items()}
    ref_state["stopping"].copy_(torch.from_numpy(ctl))
    state["stopping"].copy_(torch.from_numpy(ctl))
    x = torch.from_numpy(_prompt())
    got, ref = [], []
    for i in range(10):
        c, p = (cs[0], ps[0]) if i == 0 else (cs[1], ps[1])
        ref.append(p.reference(x if i == 0 else ref[-1].view(2, 1), state=ref_state)[1].clone())
        got.append(c((x if i == 0 else got[-1].view(2, 1)).cuda())[1].clone())
        assert torch.equal(got[-1].cpu(), ref[-1]), (i, got[-1].tolist(), ref[-1].tolist())
        assert torch.equal(state["pos"].cpu(), ref_state["pos"]) and torch.equal(state["done"].cpu(), ref_state["done"])
        assert torch.equal(state["seen"].cpu(), ref_state["seen"])
    assert state["pos"].tolist() == pos and state["done"].tolist() == [1, 1]
    assert torch.stack(got, 1).view(2, 10)[1].tolist() == [25, 153, 116, 93, 501, 312, 282, 279, 37, 46]


@pytest.mark.parametrize("kw", [dict(dtype="bf16"), dict(weights="int8", kv="int8", sampling=True)],
                         ids=["bf16", "w8-kvq8-sampling"])
def test_stopping_composes_with_the_other_tenant_options(model, kw):
    """bf16, and int8 weights with int8 caches and ``sample``: on zero control words the stopping
    tenant's logits and ids are the plain tenant's bit for bit (the penalty is an exact copy, the
    same kernels run before it); armed with the second token as the stop id, that token is
    emitted, the pad id follows and the counter stands still."""
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    x = torch.from_numpy(_prompt()).cuda()

    def run(stopping, words=None):
        progs, w = llama_decode_programs(model, PROMPT_LEN, 64, batch=2, stopping=stopping, **kw)
        ps = PG.parse_variants(progs, w, gpu=True)
        params, state, derived = ps[0].tensors("cuda"), ps[0].state_tensors("cuda"), {}
        cs = [p.compile("cuda", params=params, state=state, derived=derived) for p in ps]
        if words is not None:
            state["stopping"].copy_(torch.from_numpy(words))
        outs = [cs[0](x)]
        for _ in range(3):
            outs.append(cs[1](outs[-1][1].view(2, 1)))
        return [o[0].clone() for o in outs], torch.stack([o[1].view(2) for o in outs], 1).cpu(), state

    lg0, ids0, _ = run(False)
    lg1, ids1, st = run(True)
    assert torch.equal(ids1, ids0) and all(torch.equal(a, b) for a, b in zip(lg0, lg1))
    assert st["pos"].tolist() == [PROMPT_LEN + 3] * 2 and st["done"].tolist() == [0, 0]
    stop = int(ids0[0, 1])
    _, ids2, st = run(True, T.stopping_ctl([stop], PAD))
    want = ids0.clone()
    for r in range(2):
        hit = (ids0[r] == stop).nonzero().flatten()
        if len(hit):
            want[r, int(hit[0]) + 1:] = PAD
    h = int((ids0[0] == stop).nonzero().flatten()[0])                  # row 0's first stop: step 1, or 0 on a repeat
    assert torch.equal(ids2, want) and ids2[0, h + 1:].tolist() == [PAD] * (3 - h)
    assert st["done"][0].item() == 1 and st["pos"][0].item() == PROMPT_LEN + h


@pytest.fixture(scope="module")
def hf(model):
    """transformers on the CPU, greedy, up to 200 new tokens: per case the new ids and the smallest
    top-2 gap of the processed scores, relative to the step's max |score|, over the steps that
    decide an output (a row's steps up to the one that emits its stop id)."""
    out = {}
    for k, (eos, pen, _) in CASES.items():
        with torch.no_grad():
            g = model.generate(torch.from_numpy(_prompt()).long(), max_new_tokens=200, do_sample=False, eos_token_id=eos,
                               pad_token_id=PAD, repetition_penalty=pen if pen != 1.0 else None, output_scores=True,
                               return_dict_in_generate=True)
        ids = g.sequences[:, PROMPT_LEN:].numpy().astype(np.int32)
        gap = np.inf
        for r in range(ids.shape[0]):
            stop = np.isin(ids[r], eos)
            last = int(stop.argmax()) if stop.any() else ids.shape[1] - 1
            for i in range(last + 1):
                s = g.scores[i][r].float()
                top = torch.topk(s, 2).values
                gap = min(gap, float((top[0] - top[1]) / s.abs().max()))
        out[k] = (ids, gap)
    return out


@pytest.fixture(scope="module")
def gpu_client(tenant, tmp_path_factory):
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    srv = PodServer(tmp_path_factory.mktemp("stop") / "g.sock", device="cuda", lanes=2, memory_gb=40).start()
    try:
        c = PodClient(srv.path, connect_timeout_s=60)
        rep = c.register("stop", tenant[0][0], tenant[1], memory_limit_gb=4, variants=tenant[0][1:])
        assert rep["compile"]["stop_launches"] == 3      # the prefill's (the primary program): mark, penalise, stop step
        yield c, srv
        c.close()
    finally:
        srv.stop()


@pytest.mark.parametrize("case", sorted(CASES))
def test_gpu_server_generation_equals_transformers(case, hf, gpu_client):
    """Cases (a) and (b) through ``PodClient.generate`` on the GPU server (HIP graphs), the server
    loop and one request per token, equal to transformers on the CPU.  Equality is a fair demand:
    every deciding step's top-2 gap is at least MIN_GAP of the step's largest |score| (measured:
    2.6e-3 in (a), 9.3e-4 in (b)); (a)'s stop id ends row 1 at step 2, before its near-tie at step 4.
    (c)'s deciding steps are among (a)'s."""
    c, srv = gpu_client
    eos, pen, pos = CASES[case]
    want, gap = hf[case]
    print(f"case {case}: smallest deciding top-2 gap {gap:.3g} of max |score|")
    assert gap >= MIN_GAP, gap
    for loop in (True, False):
        ids, t = c.generate(_prompt(), 24, server_loop=loop, eos_token_id=eos, pad_token_id=PAD, repetition_penalty=pen)
        assert np.array_equal(ids, want), (loop, ids.tolist(), want.tolist())
        assert t["state"] == {"pos": pos, "done": [1, 1]}
        assert want.shape[1] - 1 <= t["steps_run"] <= 23
        if case == "c" and loop:   # the loop overran by its check windows, and the ids came back trimmed all the same
            assert want.shape == (2, 3) and want[0, 1:].tolist() == [PAD, PAD] and t["steps_run"] > 2


def test_gpu_server_early_exit_and_unarmed_requests(hf, gpu_client, model):
    c, srv = gpu_client
    eos, pen, pos = CASES["b"]
    ids, t = c.generate(_prompt(), 200, eos_token_id=eos, pad_token_id=PAD, repetition_penalty=pen)
    assert ids.shape == (2, 10) and np.array_equal(ids, hf["b"][0])
    assert 9 <= t["steps_run"] <= 9 + 2 * srv.stop_check_every and t["state"] == {"pos": pos, "done": [1, 1]}
    # no stopping field: every step runs and the tokens are transformers' plain greedy ones where
    # those are decided (the CPU server's plain run, compared in test_stopping.py, is the same function)
    plain, tp = c.generate(_prompt(), 12)
    assert plain.shape == (2, 12) and tp["steps_run"] == 11 and tp["state"] == {"pos": [17, 17], "done": [0, 0]}
    assert plain[:, :3].tolist() == [[329, 267, 63], [25, 153, 116]]
