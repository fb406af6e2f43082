"""The decode step of an int8-KV decoder beside the fp32-KV one.

One GPU pod server in this process per context, the fleet decoder (1024 hidden, 8
layers, 2 KV heads of 128, vocab 32000) registered four times -- fp32 and int8
K / V caches, each with fp32 and with int8 weights -- and ``PodClient.generate``'s
server loop run on one of them at a time, alternating.  Two contexts:

* ``max_len`` 1024, a 16-token prompt: a step is ~43 latency-bound launches;
* ``max_len`` 8192, a prompt of 4112 tokens: the loop starts past position 4096, so
  a step's bytes are mostly cache (fp32: 2 x 8 layers x 4112 rows x 1 KiB = 67 MB).

Each run is a prefill plus ``--tokens`` - 1 decode steps in one request; its figure is
the loop's wall time over its steps.  Prints, and with ``--out`` writes, per context
and tenant: ms per token (median, min, max over ``--runs``), the cache bytes a step
at the loop's middle position reads, the server's static estimate and the measured
footprint; and the one timing condition: at the long context the int8-KV tenant's
median must not exceed the fp32-KV tenant's by more than that tenant's own
run-to-run spread (max / median of its runs).

    python tools/kvq8_decode_loop.py --out profiles/kvq8_decode_loop.json
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

TENANTS = {"kv-fp32": dict(), "kv-int8": dict(kv="int8"), "w8-kv-fp32": dict(weights="int8"),
           "w8-kv-int8": dict(weights="int8", kv="int8")}


def cache_bytes_per_row(prog) -> int:
    """Bytes one cached position holds over all layers: the caches' rows and, for i8 caches, their scales."""
    return sum(v.nbytes // v.shape[1] for k, v in prog.state.items() if len(v.shape) >= 3)


def measure(m, prompt_len: int, max_len: int, a) -> dict:
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    prompt = np.random.default_rng(0).integers(0, m.config.vocab_size, (1, prompt_len)).astype(np.int32)
    times: dict[str, list[float]] = {k: [] for k in TENANTS}
    info: dict[str, dict] = {}
    with tempfile.TemporaryDirectory() as d:
        srv = PodServer(Path(d) / "s.sock", device="cuda", lanes=2, memory_gb=60).start()
        try:
            clients = {}
            for name, kw in TENANTS.items():
                progs, w = llama_decode_programs(m, prompt_len, max_len, **kw)
                ps = PG.parse_variants(progs, w, gpu=True)
                need = (sum(p.bytes_estimate_for(srv.kernel_config) for p in ps)
                        - (len(ps) - 1) * (ps[0].param_bytes + ps[0].state_bytes))
                c = clients[name] = PodClient(srv.path, connect_timeout_s=120)
                rep = c.register(name, progs[0], w, memory_limit_gb=10, variants=progs[1:])
                row = cache_bytes_per_row(ps[1])
                info[name] = {"state_bytes": ps[0].state_bytes, "cache_bytes_per_position": row,
                              "cache_bytes_read_mid_loop": row * (prompt_len + a.tokens // 2),
                              "static_estimate_gb": round(need / 2 ** 30, 4), "footprint_gb": rep["footprint_gb"]}
            for r in range(a.warmup + a.runs):
                for name in TENANTS:
                    _, tm = clients[name].generate(prompt, a.tokens)
                    if r >= a.warmup:
                        times[name].append(1e3 * tm["step_s"][0])
            for c in clients.values():
                c.close()
        finally:
            srv.stop()
    for name, v in times.items():
        info[name]["ms_per_token"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                                      "max": round(max(v), 4)}
    res = {"prompt": prompt_len, "max_len": max_len, "tenants": info}
    for pre in ("", "w8-"):
        f, q = info[pre + "kv-fp32"]["ms_per_token"], info[pre + "kv-int8"]["ms_per_token"]
        res[pre + "int8_over_fp32_kv_ms"] = round(q["median"] / f["median"], 4)
        res[pre + "fp32_kv_spread_max_over_median"] = round(f["max"] / f["median"], 4)
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("kvq8_decode_loop.py measures on the GPU: none found")
    from nos_amd.models.llama_program import llama_config, llama_model

    m = llama_model(llama_config(True), 0)
    res = {"what": "PodClient.generate's server loop, one 1024-hidden 8-layer vocab-32000 decoder alone, registered "
                   "with fp32 and int8 K / V caches (and the same pair with int8 weights): ms per token (the loop's "
                   "wall time over its steps), the tenants alternating in one process",
           "tokens": a.tokens, "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "short": measure(m, 16, 1024, a), "long": measure(m, 4112, 8192, a)}
    lg = res["long"]
    res["timing_condition"] = {
        "rule": "long context: int8-KV median <= fp32-KV median x (fp32-KV max / median)",
        "holds": lg["int8_over_fp32_kv_ms"] <= lg["fp32_kv_spread_max_over_median"],
        "holds_with_int8_weights": lg["w8-int8_over_fp32_kv_ms"] <= lg["w8-fp32_kv_spread_max_over_median"]}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
