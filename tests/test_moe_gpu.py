"""Mixture of experts on gfx950 (csrc/hip/decode.hip ``moe_route_kernel``,
``moe_glu_kernel``, ``moe_down_kernel``): each kernel against ``moe_*_ref`` in
fp64 at the project's bar (4x torch-fp32's own error, at least 2e-6 of max |y|;
model logits: at least 1e-5), then the compiled Mixtral tenant and the GPU pod
server against ``MixtralForCausalLM`` in fp64.

No input sits on a tie: the kernel tests draw seeds on the CPU until, in the
fp64 reference alone, the first min(k + 1, E) router probabilities of every row
are at least ``MIN_ROUTE_GAP`` apart (so the order of the chosen experts is
decided as clearly as the choice), and assert it; the model tests use
``test_moe``'s prompts, whose reference asserts both gaps."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402
from nos_amd.ops import _lib, _stream  # noqa: E402
from nos_amd.ops import tenant as T  # noqa: E402
from test_moe import (MAX_LEN, MIN_ROUTE_GAP, NEW, PROMPT_LEN, model, prompt, reference)  # noqa: E402, F401

SENT = 7.0
EPS = 1e-5
# rows {1, 3, 8}, E {2, 5, 8}, k {1, 2, E}, H {64, 200, 1024} (below one 256-column step, a tail, four steps),
# I {4, 100, 352} (one column group, a tail of the 4-column groups and of the 256-column steps, two steps)
SHAPES = [(1, 2, 1, 64, 4), (3, 5, 2, 200, 100), (8, 8, 8, 1024, 352), (8, 5, 5, 64, 352), (1, 8, 2, 1024, 100),
          (3, 2, 2, 200, 4)]
VARIANTS = [dict(), dict(rms_eps=EPS), dict(rms_eps=EPS, gamma=True)]


@pytest.fixture(autouse=True)
def _h3():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)


def _close(got, ref64, ref32, what, floor=2e-6) -> None:
    scale = float(ref64.abs().max()) or 1.0
    e = float((got.double().cpu() - ref64).abs().max()) / scale
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    print(f"{what}: e = {e:.3g}, e32 = {e32:.3g}")
    assert got.shape == ref64.shape and e <= max(4 * e32, floor), (what, e, e32)


def _route_gap(x, Wr, k, eps, gamma) -> float:
    """The smallest distance between neighbours among the first min(k + 1, E) sorted probabilities, fp64."""
    p = torch.softmax(T._moe_x(x, eps, gamma, torch.float64) @ Wr.double().T, -1).sort(-1, descending=True).values
    n = min(k + 1, p.shape[1])
    return float((p[:, :n - 1] - p[:, 1:n]).min()) if n > 1 else 1.0


def _inputs(rows, E, k, H, I, rms_eps=0.0, gamma=False, make_x=None):
    """CPU fp32 (x, Wr, W13, W2, gamma, res) of the first seed whose routing clears MIN_ROUTE_GAP (asserted)."""
    for seed in range(400):
        g = torch.Generator().manual_seed(1000 * rows + 100 * E + 10 * k + H + I + 7919 * seed)
        Wr = torch.randn(E, H, generator=g) / H ** 0.5
        x = torch.randn(rows, H, generator=g) if make_x is None else make_x(Wr, g)
        gm = 1 + 0.1 * torch.randn(H, generator=g) if gamma else None
        if _route_gap(x, Wr, k, rms_eps, gm) >= MIN_ROUTE_GAP:
            break
    assert _route_gap(x, Wr, k, rms_eps, gm) >= MIN_ROUTE_GAP, "no seed clears the routing gap: widen the search"
    W13 = torch.randn(E, 2 * I, H, generator=g) / H ** 0.5
    W2 = torch.randn(E, H, I, generator=g) / I ** 0.5
    res = torch.randn(rows, H, generator=g)
    return x, Wr, W13, W2, gm, res


def _padded(t: torch.Tensor, pad: tuple) -> tuple:
    """t on the GPU as a view of a sentinel-filled buffer with ``pad`` extra elements per dimension: a
    distinct leading dimension for every operand, unit inner stride, 16-byte rows.  Returns (view, buffer)."""
    buf = torch.full([s + p for s, p in zip(t.shape, pad)], SENT, device="cuda", dtype=t.dtype)
    view = buf[tuple(slice(0, s) for s in t.shape)]
    view.copy_(t)
    return view, buf


def _guarded(shape, dtype):
    """A contiguous output between two sentinel rows: (view, buffer)."""
    buf = torch.full((shape[0] + 2, *shape[1:]), 7, device="cuda", dtype=dtype)
    return buf[1:-1], buf


def _guards_intact(buf) -> bool:
    return bool((buf[0] == 7).all()) and bool((buf[-1] == 7).all())


def _run_block(x, Wr, W13, W2, gm, res, k, eps):
    """The three launches on padded operands with guarded outputs: (idx, w, act, y) and the sentinel checks."""
    rows, H = x.shape
    E, I = Wr.shape[0], W13.shape[1] // 2
    xg, _ = _padded(x, (0, 8))
    wrg, _ = _padded(Wr, (0, 4))
    w13g, _ = _padded(W13, (0, 2, 4))
    w2g, _ = _padded(W2, (0, 1, 12))
    gg = None if gm is None else gm.cuda()
    (idx, ibuf), (w, wbuf), (act, abuf) = _guarded((rows, k), torch.int32), _guarded((rows, k), torch.float32), \
        _guarded((rows, k, I), torch.float32)
    T.moe_route(xg, wrg, k, eps, gg, out=(idx, w))
    T.moe_glu(xg, idx, w13g, eps, gg, out=act)
    ys = []
    for r in (None, res):
        rg = None if r is None else _padded(r, (0, 4))[0]
        y, ybuf = _padded(torch.zeros(rows, H), (0, 4))
        ybuf.fill_(SENT)
        T.moe_down(act, idx, w, w2g, res=rg, out=y)
        assert bool((ybuf[:, H:] == SENT).all()), "moe_down wrote past its row"
        ys.append(y)
    torch.cuda.synchronize()
    assert _guards_intact(ibuf) and _guards_intact(wbuf) and _guards_intact(abuf), "a kernel wrote outside its output"
    return idx, w, act, ys[0], ys[1]


def _check_block(x, Wr, W13, W2, gm, res, k, eps, what):
    idx, w, act, y, yr = _run_block(x, Wr, W13, W2, gm, res, k, eps)
    d = torch.float64
    idx64, w64 = T.moe_route_ref(x, Wr, k, eps, gm, d)
    assert torch.equal(idx.cpu(), idx64), (what, idx.cpu().tolist(), idx64.tolist())   # the experts AND their order
    _close(w, w64, T.moe_route_ref(x, Wr, k, eps, gm)[1], (what, "route w"))
    _close(act, T.moe_glu_ref(x, idx64, W13, eps, gm, d), T.moe_glu_ref(x, idx64, W13, eps, gm), (what, "glu"))
    ac, wc = act.cpu(), w.cpu()   # the down kernel on the inputs it was given
    _close(y, T.moe_down_ref(ac, idx64, wc, W2, None, d), T.moe_down_ref(ac, idx64, wc, W2), (what, "down"))
    _close(yr, T.moe_down_ref(ac, idx64, wc, W2, res, d), T.moe_down_ref(ac, idx64, wc, W2, res), (what, "down + res"))
    # the block against the literal contract
    xp64 = T._moe_x(x, eps, gm, d)
    _close(y, T.moe_ref(xp64, Wr.double(), W13.double(), W2.double(), k),
           T.moe_ref(T._moe_x(x, eps, gm, torch.float32), Wr, W13, W2, k), (what, "block"))
    return idx, w, act, y, yr


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("rows, E, k, H, I", SHAPES)
def test_moe_kernels_match_fp64(rows, E, k, H, I):
    for v in VARIANTS:
        ins = _inputs(rows, E, k, H, I, **v)
        _check_block(*ins, k, v.get("rms_eps", 0.0), (rows, E, k, H, I, tuple(v)))


def test_two_runs_are_bit_identical():
    ins = _inputs(8, 8, 2, 1024, 352, rms_eps=EPS, gamma=True)
    a = _run_block(*ins, 2, EPS)
    b = _run_block(*ins, 2, EPS)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_every_row_the_same_expert_and_every_row_another():
    rows, E, H, I = 8, 8, 200, 100

    def same(Wr, g):   # one direction plus a little noise: every row ranks the experts alike
        return 6 * torch.randn(1, H, generator=g) + 0.001 * torch.randn(rows, H, generator=g)

    def other(Wr, g):   # row m along the router's row m: expert m first
        return 3 * Wr / Wr.pow(2).sum(-1, keepdim=True) + 0.1 * torch.randn(rows, H, generator=g)

    for k in (1, 2):
        ins = _inputs(rows, E, k, H, I, make_x=same)
        idx = _check_block(*ins, k, 0.0, ("same", k))[0].cpu()
        assert bool((idx == idx[0]).all())
        ins = _inputs(rows, E, k, H, I, make_x=other)
        idx = _check_block(*ins, k, 0.0, ("other", k))[0].cpu()
        assert idx[:, 0].tolist() == list(range(rows))


def test_unselected_experts_are_never_read():
    """Every expert no row chose holds NaN weights: the output is finite and within the bar."""
    rows, E, k, H, I = 3, 8, 2, 200, 100
    x, Wr, W13, W2, gm, res = _inputs(rows, E, k, H, I, rms_eps=EPS, gamma=True)
    chosen = set(T.moe_route_ref(x, Wr, k, EPS, gm, torch.float64)[0].flatten().tolist())
    idle = [e for e in range(E) if e not in chosen]
    assert idle
    W13n, W2n = W13.clone(), W2.clone()
    W13n[idle] = float("nan")
    W2n[idle] = float("nan")
    _, _, act, y, yr = _run_block(x, Wr, W13n, W2n, gm, res, k, EPS)
    assert bool(torch.isfinite(act).all()) and bool(torch.isfinite(y).all()) and bool(torch.isfinite(yr).all())
    xp = T._moe_x(x, EPS, gm, torch.float64)
    _close(yr, res.double() + T.moe_ref(xp, Wr.double(), W13.double(), W2.double(), k),
           res + T.moe_ref(T._moe_x(x, EPS, gm, torch.float32), Wr, W13, W2, k), "NaN experts")


def test_an_index_outside_the_experts_contributes_zero():
    rows, E, k, H, I = 3, 5, 4, 200, 100
    x, Wr, W13, W2, _, res = _inputs(rows, E, k, H, I)
    idx = torch.tensor([[1, -1, 4, E], [2 ** 30, 0, -2 ** 31, 3], [E, 64, -1, 2 ** 31 - 1]], dtype=torch.int32)
    w = torch.rand(rows, k) + 0.1
    w[2] = float("nan")   # a row with no valid slot: even its weights are never used
    xg, w13g, w2g, ig, wg = x.cuda(), W13.cuda(), W2.cuda(), idx.cuda(), w.cuda()
    act = T.moe_glu(xg, ig, w13g)
    ok = (idx >= 0) & (idx < E)
    assert bool((act.cpu()[~ok] == 0).all())
    _close(act, T.moe_glu_ref(x, idx, W13, dtype=torch.float64), T.moe_glu_ref(x, idx, W13), "glu, bad idx")
    noise = torch.where(ok.unsqueeze(-1), act.cpu(), torch.full_like(act.cpu(), float("nan")))   # their act is not read either
    y = T.moe_down(noise.cuda(), ig, wg, w2g, res=res.cuda())
    assert bool(torch.isfinite(y).all()) and torch.equal(y[2].cpu(), res[2])
    _close(y, T.moe_down_ref(act.cpu(), idx, w, W2, res, torch.float64), T.moe_down_ref(act.cpu(), idx, w, W2, res),
           "down, bad idx")


# ------------------------------------------------------------------ 2. refusals
def test_wrappers_refuse_what_the_kernels_do_not_take():
    x, Wr, W13, W2, _, _ = (t.cuda() if t is not None else None for t in _inputs(3, 5, 2, 64, 8))
    idx, w = T.moe_route(x, Wr, 2)
    act = T.moe_glu(x, idx, W13)
    wide = torch.randn(3, 72, device="cuda")
    cases = [
        lambda: T.moe_route(torch.randn(9, 64, device="cuda"), Wr, 2),             # rows
        lambda: T.moe_route(x, Wr, 0), lambda: T.moe_route(x, Wr, 6),               # k
        lambda: T.moe_route(x, torch.randn(65, 64, device="cuda"), 2),              # E
        lambda: T.moe_route(torch.randn(3, 62, device="cuda"), torch.randn(5, 62, device="cuda"), 2),   # H % 4
        lambda: T.moe_route(x.bfloat16(), Wr, 2), lambda: T.moe_route(x, Wr.double(), 2),   # dtypes
        lambda: T.moe_route(x, Wr.cpu(), 2),                                        # devices
        lambda: T.moe_route(wide[:, 1:65], Wr, 2),                                  # a misaligned base
        lambda: T.moe_route(torch.randn(3, 128, device="cuda")[:, ::2], Wr, 2),     # inner stride
        lambda: T.moe_route(torch.randn(3, 66, device="cuda")[:, :64], Wr, 2),      # a row stride off 16 bytes
        lambda: T.moe_route(x, Wr[:, :32], 2),                                      # shapes
        lambda: T.moe_route(x, Wr, 2, gamma=torch.ones(64, device="cuda")),         # gamma without rms_eps
        lambda: T.moe_glu(x, idx.long(), W13), lambda: T.moe_glu(x, idx[:2], W13),
        lambda: T.moe_glu(x, idx, W13[:, :15]), lambda: T.moe_glu(x, idx, W13.bfloat16()),
        lambda: T.moe_glu(x, idx, torch.randn(5, 12, 64, device="cuda")),           # I % 4
        lambda: T.moe_down(act, idx, w, W2[:, :, :4]), lambda: T.moe_down(act, idx, w[:, :1], W2),
        lambda: T.moe_down(act, idx, w, W2, res=torch.zeros(3, 60, device="cuda")),
        lambda: T.moe_down(act, idx, w.double(), W2), lambda: T.moe_down(act.transpose(0, 1), idx, w, W2),
        lambda: T.moe_down(act, idx, w, W2, out=torch.zeros(3, 64, device="cuda", dtype=torch.bfloat16)),
    ]
    for n, call in enumerate(cases):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {n} was taken")
    # the entry points check for themselves (hipErrorInvalidValue = 1, nothing launched)
    L = _lib.lib()
    y = torch.full((3, 64), SENT, device="cuda")
    s = _stream()
    assert L.nos_moe_route(x.data_ptr(), 64, Wr.data_ptr(), 64, None, 0.0, idx.data_ptr(), w.data_ptr(), 3, 5, 64, 6, s) == 1
    assert L.nos_moe_route(x.data_ptr(), 64, Wr.data_ptr(), 64, None, 0.0, idx.data_ptr(), w.data_ptr(), 9, 5, 64, 2, s) == 1
    assert L.nos_moe_glu(x.data_ptr(), 64, idx.data_ptr(), W13.data_ptr(), 16 * 64 - 4, 64, None, 0.0, act.data_ptr(), 3, 5,
                         64, 8, 2, s) == 1
    assert L.nos_moe_down(act.data_ptr(), idx.data_ptr(), w.data_ptr(), W2.data_ptr(), 64 * 8, 8, None, 0, y.data_ptr(), 60,
                          3, 5, 64, 8, 2, s) == 1
    assert L.nos_moe_down(act.data_ptr(), idx.data_ptr(), w.data_ptr(), W2.data_ptr() + 4, 64 * 8, 8, None, 0, y.data_ptr(),
                          64, 3, 5, 64, 8, 2, s) == 1
    torch.cuda.synchronize()
    assert bool((y == SENT).all())


# ------------------------------------------------------------------ 3. whole tenants
def _compiled(m, prompt_len: int = PROMPT_LEN, max_len: int = MAX_LEN, batch: int = 1, **kw):
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    progs, w = llama_decode_programs(m, prompt_len, max_len, batch=batch, **kw)
    ps = PG.parse_variants(progs, w, gpu=True)
    params = ps[0].tensors("cuda")
    state = ps[0].state_tensors("cuda")
    return [p.compile("cuda", params=params, state=state) for p in ps], state


def _logits_close(logits, m, seq, what) -> None:
    m = copy.deepcopy(m).cuda()
    with torch.no_grad():
        f32 = m(seq).logits[:, -1:]
        ref64 = m.double()(seq).logits[:, -1:].cpu()
    _close(logits, ref64, f32.cpu(), what, floor=1e-5)


def test_decode_step_and_prefill_logits_match_mixtral_in_fp64(model, reference):  # noqa: F811
    """The prompt and its fp64 continuation (both gaps asserted by ``reference``): a prefill of 8 rows
    (the kernels, eight rows of one sequence in every layer but the last, which keeps the last row),
    three decode steps, and a prefill of 16 rows (PyTorch ops, dense over the experts)."""
    (pre, step), state = _compiled(model)
    seq = torch.from_numpy(prompt()).long().cuda()
    with torch.no_grad():
        logits, nxt = pre(seq.int())
        _logits_close(logits, model, seq, "prefill 8")
        for s in range(3):
            assert int(nxt) == int(reference[0, s])
            seq = torch.cat([seq, nxt.long().view(1, 1)], 1)
            logits, nxt = step(nxt.view(1, 1).int())
            _logits_close(logits, model, seq, f"step {s}")
    assert state["pos"].tolist() == [PROMPT_LEN + 3]
    (pre16, _), state = _compiled(model, prompt_len=16)
    # every layer but the last, which keeps one row (the row slice moves above its moe): that one is on the kernels
    L = model.config.num_hidden_layers
    assert [s.kind for s in pre16.steps].count("moe") == L - 1 and pre16.stats["moe_launches"] == 3
    seq = torch.from_numpy(np.concatenate([prompt(), reference[:1, :8]], 1)).long().cuda()
    with torch.no_grad():
        logits, nxt = pre16(seq.int())
    _logits_close(logits, model, seq, "prefill 16")
    assert int(nxt) == int(reference[0, 8]) and state["pos"].tolist() == [16]


def test_decode_step_costs_the_dense_steps_launches_plus_one_per_layer(model):  # noqa: F811
    from nos_amd.models.llama_program import llama_config, llama_model

    cfg = model.config
    L = cfg.num_hidden_layers
    dense = llama_model(llama_config(False, hidden_size=cfg.hidden_size, num_hidden_layers=L,
                                     num_attention_heads=cfg.num_attention_heads,
                                     num_key_value_heads=cfg.num_key_value_heads, intermediate_size=cfg.intermediate_size,
                                     vocab_size=cfg.vocab_size), 0)
    (_, dstep), _ = _compiled(dense)
    (pre, step), _ = _compiled(model)
    for c in (pre, step):   # 8 rows and 1: both on the kernels
        st = c.stats
        assert st["moe_blocks"] == st["moe_rms_prologue"] == st["moe_residual_fused"] == L and st["moe_launches"] == 3 * L
        kinds = [s.kind for s in c.steps]
        assert kinds.count("moe_route") == kinds.count("moe_glu") == kinds.count("moe_down") == L
        assert "moe" not in kinds and "add" not in kinds and "rmsnorm" not in kinds
    # the route replaces nothing; glu and down take the places of the dense gate-up and down GEMVs
    assert step.stats["kernels"] == dstep.stats["kernels"] + L
    assert dstep.stats["moe_blocks"] == dstep.stats["moe_launches"] == 0
    assert step.stats["rmsnorm_folded"] == dstep.stats["rmsnorm_folded"] - L   # those norms are the moe prologues
    for k in ("decode_combines_into_gemv", "kv_writes_into_attention", "pos_add_into_argmax", "rotary_at_fused"):
        assert step.stats.get(k) == dstep.stats.get(k), k
    # no derived copy of an expert weight: the steps read the params themselves
    for s in step.steps:
        if s.kind in ("moe_glu", "moe_down"):
            assert s.inputs[2].endswith(("experts.gate_up_proj", "experts.down_proj")) and s.inputs[2] in step.consts


def test_gpu_server_generates_mixtrals_tokens(model, reference, tmp_path):  # noqa: F811
    """HIP graphs and the server loop, batch 2 and a speculating tenant, token for token."""
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    srv = PodServer(tmp_path / "g.sock", device="cuda", lanes=2, memory_gb=40).start()
    try:
        progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN)
        c = PodClient(srv.path, connect_timeout_s=60)
        c.register("moe", progs[0], w, memory_limit_gb=4, variants=progs[1:])
        for loop in (True, False):
            ids, tm = c.generate(prompt(), NEW, server_loop=loop)
            assert np.array_equal(ids, reference[:1]), (loop, ids, reference[:1])
            assert tm["state"] == {"pos": [PROMPT_LEN + NEW - 1]}
        c.close()
        progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, batch=2)
        c = PodClient(srv.path, connect_timeout_s=60)
        c.register("moe-b2", progs[0], w, memory_limit_gb=4, variants=progs[1:])
        got, _ = c.generate(prompt(2), NEW, server_loop=True)
        assert np.array_equal(got, reference), (got, reference)
        c.close()
        progs, w = llama_decode_programs(model, PROMPT_LEN, MAX_LEN, speculate=4)
        c = PodClient(srv.path, connect_timeout_s=60)
        c.register("moe-spec", progs[0], w, memory_limit_gb=4, variants=progs[1:])
        spec, _ = c.generate(prompt(), NEW, speculate=True)
        assert np.array_equal(spec, reference[:1]), (spec, reference[:1])
        c.close()
    finally:
        srv.stop()
