#!/usr/bin/env python
"""Chunked prefill on the flash kernel against the decode kernel: ms per ``extend`` chunk of the fleet decoder
(1024 hidden, 8 layers, G = 4) with ``max_len`` 8192 plain caches and with ``window=1024`` rings, at chunk
lengths 16 / 64 / 256 starting at positions 0 / 2048 / 6144, and the time to first token of a 4096-token prompt
fed as 64-token chunks.

Both paths live in one process: the tenant is compiled twice over the same weights and state, once as it is and
once under ``NOS_AMD_CACHE_FLASH=0`` (the parent's path: the decode kernel on every step), and the two are
alternated run by run.  A run is one captured graph of the step (what the server replays), timed with events;
the counter is set on the device before it.  Median of ``--runs`` with min and max; the decode path's max /
median is the spread a win has to beat.  Writes ``profiles/extend_flash_loop.json``."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

CHUNKS = (16, 64, 256)
STARTS = (0, 2048, 6144)
MAX_LEN = 8192


def compile_both(model, device="cuda"):
    """{path: {chunk: compiled step}} over one set of weights and one state, and that state."""
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    progs, w = llama_decode_programs(model, 8, MAX_LEN, extend=CHUNKS)
    ps = PG.parse_variants(progs, w, gpu=True)
    params, state = ps[0].tensors(device), ps[0].state_tensors(device)
    out = {}
    for path, env in (("flash", None), ("decode", "0")):
        if env is None:
            os.environ.pop("NOS_AMD_CACHE_FLASH", None)
        else:
            os.environ["NOS_AMD_CACHE_FLASH"] = env
        out[path] = {p.inputs[0].shape[1]: p.compile(device, params=params, state=state) for p in ps
                     if p.inputs[0].shape[1] in CHUNKS + (1,)}
    os.environ.pop("NOS_AMD_CACHE_FLASH", None)
    return out, state


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def measure(model, runs: int, ttft_tokens: int):
    import torch

    both, state = compile_both(model)
    g = torch.Generator(device="cuda").manual_seed(0)
    for k, t in state.items():      # full caches: the decode path reads whatever they hold
        if t.dtype == torch.float32:
            t.copy_(torch.randn(t.shape, device="cuda", generator=g))
    side = torch.cuda.Stream()
    rows = []
    for n in CHUNKS:
        x = torch.randint(0, model.config.vocab_size, (1, n), device="cuda", dtype=torch.int32, generator=g)
        graphs = {}
        for path in both:
            with torch.no_grad(), torch.cuda.stream(side):
                state["pos"].fill_(0)
                both[path][n](x)
                side.synchronize()
                graphs[path] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[path], stream=side):
                    both[path][n](x)
        for p0 in STARTS:
            ms = {path: [] for path in both}
            for r in range(runs + 1):           # the first round warms up
                for path in both:
                    state["pos"].fill_(p0)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    graphs[path].replay()
                    b.record()
                    b.synchronize()
                    if r:
                        ms[path].append(a.elapsed_time(b))
            row = {"chunk": n, "start": p0, "ms": {k: stat(v) for k, v in ms.items()},
                   "flash_step": bool(both["flash"][n].stats["flash_cache"]),
                   "launches": {k: both[k][n].stats["kernels"] for k in both}}
            d = row["ms"]["decode"]
            row["decode_spread"] = round(d["max"] / d["median"], 4)
            row["decode_over_flash"] = round(d["median"] / row["ms"]["flash"]["median"], 4)
            row["flash_wins"] = row["decode_over_flash"] > row["decode_spread"]
            rows.append(row)
            print(json.dumps(row), flush=True)
        del graphs
    # time to first token: the prompt as 64-token chunks from position 0, the launches enqueued eagerly
    x = torch.randint(0, model.config.vocab_size, (1, 64), device="cuda", dtype=torch.int32, generator=g)
    ttft = {path: [] for path in both}
    for r in range(4):
        for path in both:
            state["pos"].fill_(0)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            with torch.no_grad():
                for _ in range(ttft_tokens // 64):
                    both[path][64](x)
            b.record()
            b.synchronize()
            if r:
                ttft[path].append(a.elapsed_time(b))
    one = {}
    for path in both:                    # the one-token step is the same program on both paths
        state["pos"].fill_(2048)
        tok = torch.zeros(1, 1, device="cuda", dtype=torch.int32)
        v = []
        for r in range(runs + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            with torch.no_grad():
                for _ in range(32):
                    both[path][1](tok)
            b.record()
            b.synchronize()
            if r:
                v.append(a.elapsed_time(b) / 32)
        one[path] = stat(v)
    return {"chunks": rows, "ttft_ms": {k: stat(v) for k, v in ttft.items()}, "ttft_tokens": ttft_tokens,
            "one_token_ms": one,
            "one_token_step_identical": [s.kind for s in both["flash"][1].steps] == [s.kind for s in both["decode"][1].steps]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--ttft-tokens", type=int, default=4096)
    ap.add_argument("--out", default=str(REPO / "profiles" / "extend_flash_loop.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("extend_flash_loop.py measures on the GPU: none found")
    from nos_amd import ops
    from nos_amd.models.llama_program import llama_config, llama_model, mistral_config, mistral_model
    from nos_amd.ops.tenant import DECODE_MAX_ROWS

    torch.backends.cuda.matmul.allow_tf32 = False
    ops.set_f32_math("h3")
    out = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "max_len": MAX_LEN,
           "rule": f"G x Sq > {DECODE_MAX_ROWS}", "tenants": {}}
    for name, model in (("llama_plain", llama_model(llama_config(True, max_position_embeddings=MAX_LEN), 0)),
                        ("mistral_window_1024", mistral_model(mistral_config(False), 0))):
        out["tenants"][name] = measure(model, a.runs, a.ttft_tokens)
        del model
        torch.cuda.empty_cache()
    sel = [r for t in out["tenants"].values() for r in t["chunks"] if r["flash_step"]]
    out["every_selected_chunk_wins"] = all(r["flash_wins"] for r in sel)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"every_selected_chunk_wins": out["every_selected_chunk_wins"],
                      "ttft_ms": {k: t["ttft_ms"] for k, t in out["tenants"].items()}}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
