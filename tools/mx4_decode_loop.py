"""The decode step of an MXFP4 weight-only decoder beside the int8 and the fp32 one.

One GPU pod server in this process, the fleet decoder (1024 hidden, 8 layers,
vocab 32000, K / V caches of ``--max-len`` 1024 rows) registered three times --
fp32 weights, ``weights="int8"`` and ``weights="mxfp4"`` -- and
``PodClient.generate``'s server loop run on one of them at a time, alternating.
Each run is a prefill plus ``--tokens`` - 1 decode steps in one request; its
figure is the loop's wall time over its steps.  Prints, and with ``--out`` writes:

* ms per token of each tenant (median, min, max over ``--runs``) and the ratios;
* per tenant: the launches of a decode step (the compiled step's native kernels),
  the weight bytes it streams, from the decode program itself (every param a
  ``linear`` / ``linear_q8`` / ``linear_mx4`` / ``rmsnorm`` node reads), the payload
  bytes, the server's static estimate and the measured ``footprint_gb``;
* each GEMV kernel alone at M = 1, MXFP4 against int8, at the decode step's
  linear shapes and at N = 16384, K = 8192: microseconds per launch between
  device events around one captured graph of the window's launches, which
  rotate over copies of the weight (512 MB of int8 copies or 64 of them,
  whichever is less) so that no launch re-reads what the one before it left in
  the caches.

The memory figures are asserted (an MXFP4 linear streams 17 / 32 of a byte per
weight, against int8's byte plus 4 bytes a row); the times are reported.

    python tools/mx4_decode_loop.py --out profiles/mx4_decode_loop.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

LINEARS = ("linear", "linear_q8", "linear_mx4")


def streamed_bytes(prog) -> int:
    """Bytes of the params a step reads in full: its linears' weights (and scales, biases) and its
    norms' gammas (the embedding gathers one row)."""
    names = {i for n in prog.nodes if n.op in (*LINEARS, "rmsnorm") for i in n.inputs[1:]}
    return sum(prog.params[i].nbytes for i in names if i in prog.params)


def linear_shapes(prog) -> list[tuple[int, int]]:
    """(N, K) of every linear of the step, in program order."""
    return [(prog.values[n.inputs[1]].shape[0], prog.values[n.inputs[0]].shape[-1]) for n in prog.nodes
            if n.op in LINEARS]


def check_bytes(steps: dict) -> dict:
    """The format's claim, from the programs' params: per linear, MXFP4 holds N K / 2 + N K / 32 bytes
    and int8 N K + 4 N; everything else a step streams (the gammas) is the same in both."""
    shapes = linear_shapes(steps["mxfp4"])
    assert shapes == linear_shapes(steps["int8"]), "the two quantized steps hold the same linears"
    nk, rows = sum(n * k for n, k in shapes), sum(n for n, _ in shapes)
    other = streamed_bytes(steps["int8"]) - (nk + 4 * rows)
    assert other >= 0 and streamed_bytes(steps["mxfp4"]) == nk * 17 // 32 + other, "MXFP4 streams 17 / 32 byte a weight"
    ratio = streamed_bytes(steps["mxfp4"]) / streamed_bytes(steps["int8"])
    assert ratio < 17 / 32 + 1e-3, ratio
    return {"linear_weights": nk, "linear_rows": rows, "other_streamed_bytes": other,
            "mxfp4_over_int8_streamed_bytes": round(ratio, 4)}


def gemv_alone(shapes: list[tuple[int, int]], reps: int = 5) -> list[dict]:
    import torch

    from nos_amd.ops import tenant as T

    out = []
    for N, K in shapes:
        copies = max(2, min(64, -(-(512 << 20) // (N * K))))
        g = torch.Generator(device="cuda").manual_seed(N + K)
        q8 = [torch.randint(-127, 128, (N, K), generator=g, device="cuda", dtype=torch.int32).to(torch.int8)
              for _ in range(copies)]
        s8 = torch.rand(N, generator=g, device="cuda") / K
        m4 = [torch.randint(0, 256, (N, K // 2), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
              for _ in range(copies)]
        e4 = [torch.randint(110, 121, (N, K // 32), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
              for _ in range(copies)]
        x = torch.randn(1, K, generator=g, device="cuda")
        iters = 1000 if N * K < (16 << 20) else 200
        runs = {"int8": lambda i: T.gemv_q8(x, q8[i % copies], s8), "mxfp4": lambda i: T.gemv_mx4(x, m4[i % copies], e4[i % copies])}
        us: dict[str, list[float]] = {k: [] for k in runs}
        # the launches of a window as one captured graph (what the server replays): the host's
        # enqueue rate, about 11 us a launch from Python, would otherwise be the figure
        graphs = {}
        side = torch.cuda.Stream()
        for kind, run in runs.items():
            with torch.cuda.stream(side):
                for i in range(copies):
                    run(i)
            side.synchronize()
            graphs[kind] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[kind], stream=side):
                for i in range(iters):
                    run(i)
        for r in range(reps + 1):   # the first round warms up
            for kind in runs:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                graphs[kind].replay()
                b.record()
                b.synchronize()
                if r:
                    us[kind].append(1e3 * a.elapsed_time(b) / iters)
        del graphs
        row = {"N": N, "K": K, "copies": copies, "launches_per_window": iters,
               "us_per_launch": {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
                                     "max": round(max(v), 3)} for k, v in us.items()},
               "weight_bytes": {"int8": N * K + 4 * N, "mxfp4": N * K // 2 + N * K // 32}}
        row["mxfp4_over_int8_us"] = round(row["us_per_launch"]["mxfp4"]["median"] / row["us_per_launch"]["int8"]["median"], 4)
        out.append(row)
        del q8, m4, e4
        torch.cuda.empty_cache()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prompt", type=int, default=16)
    ap.add_argument("--max-len", type=int, default=1024)
    ap.add_argument("--kernels-only", action="store_true", help="only the GEMV kernels alone (an A/B of two builds)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("mx4_decode_loop.py measures on the GPU: none found")
    from nos_amd.models.llama_program import llama_config, llama_decode_programs, llama_model
    from nos_amd.podserver import program as PG
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    m = llama_model(llama_config(True), 0)
    prompt = np.random.default_rng(0).integers(0, m.config.vocab_size, (1, a.prompt)).astype(np.int32)
    kinds = ("fp32", "int8", "mxfp4")
    times: dict[str, list[float]] = {k: [] for k in kinds}
    info: dict[str, dict] = {}
    steps = {}
    res: dict = {}
    if a.kernels_only:
        progs, w = llama_decode_programs(m, a.prompt, a.max_len, weights="mxfp4")
        steps["mxfp4"] = PG.parse_variants(progs, w, gpu=True)[1]
    else:
        with tempfile.TemporaryDirectory() as d:
            srv = PodServer(Path(d) / "s.sock", device="cuda", lanes=2, memory_gb=40).start()
            try:
                clients = {}
                for kind in kinds:
                    progs, w = llama_decode_programs(m, a.prompt, a.max_len, weights=kind)
                    ps = PG.parse_variants(progs, w, gpu=True)
                    steps[kind] = ps[1]
                    need = (sum(p.bytes_estimate_for(srv.kernel_config) for p in ps)
                            - (len(ps) - 1) * (ps[0].param_bytes + ps[0].state_bytes))
                    step = ps[1].compile("cuda", params=ps[0].tensors("cuda"))
                    launches = step.stats["kernels"]
                    del step
                    torch.cuda.empty_cache()
                    c = clients[kind] = PodClient(srv.path, connect_timeout_s=60)
                    rep = c.register(kind, progs[0], w, memory_limit_gb=8, variants=progs[1:])
                    info[kind] = {"launches_per_step": launches, "payload_bytes": len(w), "param_bytes": ps[0].param_bytes,
                                  "streamed_bytes_per_token": streamed_bytes(ps[1]),
                                  "static_estimate_gb": round(need / 2 ** 30, 4), "footprint_gb": rep["footprint_gb"]}
                for r in range(a.warmup + a.runs):
                    for kind in kinds:
                        _, tm = clients[kind].generate(prompt, a.tokens)
                        if r >= a.warmup:
                            times[kind].append(1e3 * tm["step_s"][0])
                for c in clients.values():
                    c.close()
            finally:
                srv.stop()
        res = {"what": "PodClient.generate's server loop, one 1024-hidden 8-layer vocab-32000 decoder alone, registered "
                       "with fp32, int8 and MXFP4 weights: ms per token (the loop's wall time over its steps), the three "
                       "alternating in one process; then the int8 and MXFP4 GEMV kernels alone at M = 1",
               "tokens": a.tokens, "prompt": a.prompt, "max_len": a.max_len, "runs": a.runs, "warmup": a.warmup,
               "device": torch.cuda.get_device_name(0),
               "ms_per_token": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                                    "max": round(max(v), 4)} for k, v in times.items()},
               "tenants": info, "bytes": check_bytes(steps)}
        for k in kinds:
            info[k]["tb_per_s_at_median"] = round(info[k]["streamed_bytes_per_token"]
                                                  / (res["ms_per_token"][k]["median"] * 1e-3) / 1e12, 4)
        med = {k: res["ms_per_token"][k]["median"] for k in kinds}
        res["mxfp4_over_int8_ms"] = round(med["mxfp4"] / med["int8"], 4)
        res["mxfp4_over_fp32_ms"] = round(med["mxfp4"] / med["fp32"], 4)
    shapes = list(dict.fromkeys(linear_shapes(steps["mxfp4"]))) + [(16384, 8192)]
    res["gemv_alone_m1"] = gemv_alone(shapes)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
