"""The sampling kernel (csrc/hip/decode.hip ``sample_kernel``) against the
CPU reference of ``ops.tenant.sample`` token for token, and sampled
generation on the GPU pod server against the CPU server's.

The kernel scores in fp32, the reference in fp64: a draw whose two best
reference scores are closer than 1e-3 may legitimately differ and is left
out, as is a top-p row with a token whose mass-above ratio lies within 1e-4
of top_p; every other draw must be equal, and at most 1 % may be left out
(the top-p inputs are chosen so that their rule leaves none out)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nos_amd import ops  # noqa: E402
from nos_amd.ops import tenant as T  # noqa: E402

KP = [(0, 1.0), (50, 1.0), (0, 0.9), (50, 0.9), (1, 0.5)]
GAP, P_MARGIN = 1e-3, 1e-4


@pytest.fixture(autouse=True)
def _h3():
    torch.backends.cuda.matmul.allow_tf32 = False
    prev = ops.f32_math()
    ops.set_f32_math("h3")
    yield
    ops.set_f32_math(prev)


def _ctl(*a) -> torch.Tensor:
    return torch.from_numpy(T.sampling_ctl(*a)).cuda()


def _randn(rows, L, seed, top=None, bf16=False):
    """``rows`` rows of logits (randn x 2, a fixed generator).  ``top`` =
    (temperature, k, p) with p < 1: the top-p inputs are chosen so that the
    boundary rule leaves no draw out -- of four times as many candidates, the
    first whose boundary (by the reference) is clear of every token by
    2 x P_MARGIN; without top-k the logits are randn x 6, or the tokens at
    the boundary of a 1000-token nucleus weigh less than P_MARGIN each and
    no row is clear."""
    if not top or top[2] >= 1:
        x = torch.randn(rows, L, generator=torch.Generator().manual_seed(seed)) * 2.0
        return x.bfloat16() if bf16 else x
    x = torch.randn(4 * rows + 4, L, generator=torch.Generator().manual_seed(seed)) * (2.0 if top[1] else 6.0)
    x = x.bfloat16() if bf16 else x
    ctl = T.sampling_ctl(*top, 0)
    ok = [r for r in range(x.shape[0]) if T.sample_row_ref(x[r].float().numpy(), ctl)["p_margin"] >= 2 * P_MARGIN]
    assert len(ok) >= rows, (L, top, len(ok))
    return x[ok[:rows]]


def _compare(x: torch.Tensor, temp, k, p, seed, pos=None, pad=0) -> tuple[int, int, int]:
    """x on the CPU (``pad``: given to the kernel as a column slice of rows
    2 x pad longer): (draws, left out by the score gap, left out by the top-p
    boundary); asserts every other draw equal."""
    rows, L = x.shape
    ctl = T.sampling_ctl(temp, k, p, seed)
    xg = x.cuda()
    if pad:
        xg = torch.nn.functional.pad(x, (pad, pad), value=99.0).cuda()[:, pad:pad + L]
    pg = None if pos is None else torch.tensor(pos, dtype=torch.int32).cuda()
    got = T.sample(xg, torch.from_numpy(ctl).cuda(), pg).cpu().tolist()
    xs = x.float().numpy()
    n_gap = n_p = 0
    for r in range(rows):
        ref = T.sample_row_ref(xs[r], ctl, r, 0 if pos is None else pos[r])
        if ref["p_margin"] < P_MARGIN:
            n_p += 1
        elif ref["gap"] < GAP:
            n_gap += 1
        else:
            assert got[r] == ref["token"], (tuple(x.shape), temp, k, p, r, got[r], ref["token"], ref["gap"])
    return rows, n_gap, n_p


def test_greedy_is_argmax():
    """ctl zeros, and T = 0 with the other words set: nos_argmax's result on
    its own test's inputs; top_k = 1 with a unique maximum too."""
    zeros = torch.zeros(4, dtype=torch.int32, device="cuda")
    t0 = torch.tensor([0, 7, 0x3F000000, 99], dtype=torch.int32, device="cuda")
    x = torch.randn(7, 32000, device="cuda")
    x[2, 100] = x[2, 31999] = 50.0
    xb = x.bfloat16()
    for ctl in (zeros, t0):
        assert torch.equal(T.sample(x, ctl), T.argmax(x)) and torch.equal(T.sample(xb, ctl), T.argmax(xb))
    x[5, 7] = x[5, 30000] = float("nan")
    x[6] = float("-inf")
    short = torch.randn(3, 1000, device="cuda")
    for ctl in (zeros, t0, _ctl(0.9, 40, 0.9, 5)):      # a NaN or infinite maximum is greedy at any temperature
        assert T.sample(x, ctl).tolist()[5:] == [7, 0]
    for ctl in (zeros, t0):
        assert torch.equal(T.sample(short, ctl), T.argmax(short))
        p3 = torch.tensor([4, 0, 9], dtype=torch.int32, device="cuda")
        assert torch.equal(T.sample(short, ctl, pos=p3, pos_n=2), T.argmax(short)) and p3.tolist() == [6, 2, 11]
    top1 = _ctl(1.0, 1, 1.0, 3)
    assert torch.equal(T.sample(short, top1), T.argmax(short)) and torch.equal(T.sample(x[3:5], top1), T.argmax(x[3:5]))
    with pytest.raises(ValueError):
        T.sample(short, zeros.cpu())
    with pytest.raises(ValueError):
        T.sample(short, zeros, pos=torch.zeros(2, dtype=torch.int32, device="cuda"))


def test_draws_equal_the_reference_token_for_token():
    tally = np.zeros(3, dtype=np.int64)
    seed = 0
    for L, kps in ((1000, KP), (4099, [(50, 0.9), (0, 1.0)]), (32000, [(50, 0.9), (0, 1.0)])):
        for rows in (1, 3):
            for temp in (0.7, 1.3):
                for k, p in kps:
                    seed += 1
                    tally += _compare(_randn(rows, L, 100 + L + rows, (temp, k, p)), temp, k, p, seed, pos=list(range(5, 5 + rows)))
    # bf16 logits (ties by the dozen: equal logits stay or go together), and rows that are a column slice
    tally += _compare(_randn(3, 4099, 7, (0.7, 50, 0.9), bf16=True), 0.7, 50, 0.9, 11, pos=[0, 1, 2])
    tally += _compare(_randn(3, 1000, 8, (1.3, 50, 0.9)), 1.3, 50, 0.9, 12, pos=[3, 3, 3], pad=150)
    # a run of -inf logits; a tie exactly at the k-th value (both stay); without pos the counter is 0
    x = _randn(2, 1000, 13)     # (both rows clear of the top-p boundary: n_p below)
    x[0, 100:300] = float("-inf")
    order = x[1].argsort(descending=True)
    x[1, order[50]] = x[1, order[49]]
    assert T.sample_row_ref(x[1].numpy(), T.sampling_ctl(0.7, 50, 1.0, 1))["keep"].sum() == 51
    for k, p in ((50, 1.0), (0, 0.9), (50, 0.9), (900, 1.0)):
        tally += _compare(x, 0.7, k, p, 13)
    # a large vocabulary
    tally += _compare(_randn(1, 128256, 10, (0.7, 50, 0.9)), 0.7, 50, 0.9, 14, pos=[77])
    tally += _compare(_randn(1, 128256, 10), 1.3, 0, 1.0, 15, pos=[78])
    draws, n_gap, n_p = tally
    assert n_p == 0 and n_gap <= 0.01 * draws, tally


def test_draws_of_2048_rows_equal_the_reference():
    rows = 2048
    pos = [(37 * r) % 1000 for r in range(rows)]
    draws, n_gap, n_p = _compare(_randn(rows, 1000, 21), 0.7, 50, 1.0, 4321, pos=pos)
    assert n_p == 0 and n_gap <= 0.01 * draws, (n_gap, n_p)


def test_draws_repeat_and_are_keyed_on_seed_position_and_row():
    rows = 512
    x = _randn(1, 1000, 31, (0.8, 50, 0.9)).expand(rows, 1000).contiguous().cuda()
    pos = torch.arange(rows, dtype=torch.int32, device="cuda")
    for a in ((1.0, 0, 1.0), (0.8, 50, 0.9)):
        base = T.sample(x, _ctl(*a, 5), pos)
        assert torch.equal(T.sample(x, _ctl(*a, 5), pos), base)                      # bit for bit
        assert (T.sample(x, _ctl(*a, 6), pos) != base).sum() > rows // 2             # the seed
        assert (T.sample(x, _ctl(*a, 5), pos + 1) != base).sum() > rows // 2         # the position
        same_pos = T.sample(x, _ctl(*a, 5), torch.zeros_like(pos))                   # the row alone
        assert (same_pos[1:] != same_pos[:-1]).sum() > rows // 2
    p2 = pos.clone()
    assert torch.equal(T.sample(x, _ctl(1.0, 0, 1.0, 5), p2, pos_n=3), T.sample(x, _ctl(1.0, 0, 1.0, 5), pos))
    assert torch.equal(p2, pos + 3)                                                  # the counter before the advance keys


def test_sampling_decoder_on_the_gpu_server(tmp_path, monkeypatch):
    """The tiny decoder with sampling programs: the closing pos_add inside
    the sample launch, and 16 sampled tokens on the GPU pod server equal to
    the CPU server's (each step under the score-gap rule; after the first
    step left out the sequences may part, so the comparison stops there)."""
    from nos_amd.models.llama_program import llama_config, llama_decode_programs, llama_model
    from nos_amd.podserver import program as PG
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    m = llama_model(llama_config(False), 0)
    progs, w = llama_decode_programs(m, 8, 64, sampling=True)
    gprogs, gw = llama_decode_programs(m, 8, 64)
    ps = PG.parse_variants(progs, w, gpu=True)
    params = ps[0].tensors("cuda")
    c = ps[1].compile("cuda", params=params)
    greedy = PG.parse_variants(gprogs, gw, gpu=True)[1].compile("cuda", params=params)
    assert c.stats["pos_add_into_sample"] == 1 and c.stats["pos_add_into_argmax"] == 0
    assert "pos_add_into_sample" not in greedy.stats and c.stats["kernels"] == greedy.stats["kernels"]
    assert [s.kind for s in c.steps].count("sample") == 1 and "pos_add" not in [s.kind for s in c.steps]
    monkeypatch.setenv("NOS_AMD_SKIP_PASSES", "argmax_pos")
    unfused = ps[1].compile("cuda", params=params)
    monkeypatch.delenv("NOS_AMD_SKIP_PASSES")
    assert unfused.stats["kernels"] == c.stats["kernels"] + 1 and "pos_add" in [s.kind for s in unfused.steps]

    kw = dict(temperature=0.8, top_k=20, seed=3)
    ctl = T.sampling_ctl(**kw)
    prompt = np.random.default_rng(4).integers(0, m.config.vocab_size, (1, 8)).astype(np.int32)
    servers = [PodServer(tmp_path / f"{d}.sock", device=d, lanes=2, memory_gb=40).start() for d in ("cpu", "cuda")]
    try:
        cpu, gpu, plain = (PodClient(s.path, connect_timeout_s=60) for s in (servers[0], servers[1], servers[1]))
        for cl in (cpu, gpu):
            cl.register("llm", progs[0], w, memory_limit_gb=4, variants=progs[1:])
        plain.register("greedy", gprogs[0], gw, memory_limit_gb=4, variants=gprogs[1:])
        ids, tm = gpu.generate(prompt, 16, **kw)
        assert tm["state"] == {"pos": [8 + 15]}
        assert np.array_equal(gpu.generate(prompt, 16, server_loop=False, **kw)[0], ids)
        # the CPU server token by token, with each step's logits for the score gap
        x, compared = prompt, 0
        for i in range(16):
            outs, rep = cpu.infer(x, outputs=True, sampling=kw)
            ref = T.sample_row_ref(outs[0].reshape(-1), ctl, 0, rep["state"]["pos"][0] - x.shape[1])
            assert ref["token"] == int(outs[1].reshape(-1)[0])
            if ref["gap"] < GAP:
                break
            assert ids[0, i] == ref["token"], (i, ids, ref["token"])
            compared += 1
            x = np.array([[ref["token"]]], np.int32)
        assert compared >= 8, compared       # fixed inputs: most of the sequence is compared
        assert np.array_equal(gpu.generate(prompt, 16)[0], plain.generate(prompt, 16)[0])   # no parameters: greedy
        for cl in (cpu, gpu, plain):
            cl.close()
    finally:
        for s in servers:
            s.stop()
