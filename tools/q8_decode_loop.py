"""The decode step of an int8 weight-only decoder beside the fp32 one.

One GPU pod server in this process, the fleet decoder (1024 hidden, 8 layers,
vocab 32000, K / V caches of ``--max-len`` 1024 rows) registered twice -- with
fp32 weights and with ``weights="int8"`` -- and ``PodClient.generate``'s
server loop run on one of them at a time, alternating.  Each run is a prefill
plus ``--tokens`` - 1 decode steps in one request; its figure is the loop's
wall time over its steps.  Prints, and with ``--out`` writes:

* ms per token of each tenant (median, min, max over ``--runs``) and the ratio;
* the weight bytes one decode step streams, from the decode program itself
  (every param a ``linear`` / ``linear_q8`` / ``rmsnorm`` node reads), and the
  TB/s that makes at the median step;
* each tenant's measured ``footprint_gb`` and the server's static estimate.

    python tools/q8_decode_loop.py --out profiles/q8_decode_loop.json
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


def streamed_bytes(prog) -> int:
    """Bytes of the params a step reads in full: its linears' weights (and row
    scales, biases) and its norms' gammas (the embedding gathers one row)."""
    names = {i for n in prog.nodes if n.op in ("linear", "linear_q8", "rmsnorm") for i in n.inputs[1:]}
    return sum(prog.params[i].nbytes for i in names if i in prog.params)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prompt", type=int, default=16)
    ap.add_argument("--max-len", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("q8_decode_loop.py measures on the GPU: none found")
    from nos_amd.models.llama_program import llama_config, llama_decode_programs, llama_model
    from nos_amd.podserver import program as PG
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    m = llama_model(llama_config(True), 0)
    prompt = np.random.default_rng(0).integers(0, m.config.vocab_size, (1, a.prompt)).astype(np.int32)
    kinds = ("fp32", "int8")
    times: dict[str, list[float]] = {k: [] for k in kinds}
    info: dict[str, dict] = {}
    with tempfile.TemporaryDirectory() as d:
        srv = PodServer(Path(d) / "s.sock", device="cuda", lanes=2, memory_gb=40).start()
        try:
            clients = {}
            for kind in kinds:
                progs, w = llama_decode_programs(m, a.prompt, a.max_len, weights=kind)
                ps = PG.parse_variants(progs, w, gpu=True)
                need = (sum(p.bytes_estimate_for(srv.kernel_config) for p in ps)
                        - (len(ps) - 1) * (ps[0].param_bytes + ps[0].state_bytes))
                c = clients[kind] = PodClient(srv.path, connect_timeout_s=60)
                rep = c.register(kind, progs[0], w, memory_limit_gb=8, variants=progs[1:])
                info[kind] = {"payload_bytes": len(w), "param_bytes": ps[0].param_bytes,
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
                   "with fp32 and with int8 weights: ms per token (the loop's wall time over its steps), the two "
                   "alternating in one process",
           "tokens": a.tokens, "prompt": a.prompt, "max_len": a.max_len, "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0),
           "ms_per_token": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                                "max": round(max(v), 4)} for k, v in times.items()},
           "tenants": info}
    for k in kinds:
        info[k]["tb_per_s_at_median"] = round(info[k]["streamed_bytes_per_token"]
                                              / (res["ms_per_token"][k]["median"] * 1e-3) / 1e12, 4)
    res["int8_over_fp32_ms"] = round(res["ms_per_token"]["int8"]["median"] / res["ms_per_token"]["fp32"]["median"], 4)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
