"""The decode step of a sliding-window decoder on ring K / V caches beside the full-cache one.

One GPU pod server in this process, the fleet decoder (1024 hidden, 8 layers, 2 KV heads of
128, vocab 32000) registered three times:

* ``full-8192``: ``max_len`` 8192, full caches (``[1, 8192, 2, 128]`` per layer and K / V);
* ``swa-8192``: ``max_len`` 8192 with a window of 1024 -- ring caches of ``1024 + 64 - 1`` slots;
* ``full-1024``: ``max_len`` 1024, full caches.

Every tenant takes its context as a 32-token prefill and 64-token extend chunks (the ring is
sized by the longest step, so a long prompt goes in as chunks).  The two ``max_len`` 8192
tenants are filled to position 4128 and then run ``PodClient.generate``'s server loop for
``--tokens`` tokens, alternating; ``full-1024`` is filled to position 736, so that its loop
ends below its 1024 rows.  A run's figure is the loop's wall time over its steps.

Prints, and with ``--out`` writes, per tenant: ms per token (median, min, max over ``--runs``),
the launches of a decode step, the cache bytes, the server's static estimate and the measured
footprint.  Nothing is gated on the times.  The memory figures are the claim: the ring tenant's
cache bytes are ``C / max_len`` of the full tenant's (asserted here).

    python tools/swa_decode_loop.py --out profiles/swa_decode_loop.json
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

PREFILL, CHUNK = 32, 64
TENANTS = {"full-8192": dict(max_len=8192, window=None, start=PREFILL + 64 * CHUNK),
           "swa-8192": dict(max_len=8192, window=1024, start=PREFILL + 64 * CHUNK),
           "full-1024": dict(max_len=1024, window=None, start=PREFILL + 11 * CHUNK)}


def cache_bytes(prog) -> int:
    """The K / V caches' bytes over all layers (and, for i8 caches, their scales')."""
    return sum(v.nbytes for k, v in prog.state.items() if len(v.shape) >= 3)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("swa_decode_loop.py measures on the GPU: none found")
    from nos_amd.models.llama_program import llama_config, llama_decode_programs, llama_model
    from nos_amd.podserver import program as PG
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    m = llama_model(llama_config(True, max_position_embeddings=8192), 0)
    ids = np.random.default_rng(0).integers(0, m.config.vocab_size, (1, PREFILL + 64 * CHUNK)).astype(np.int32)
    times: dict[str, list[float]] = {k: [] for k in TENANTS}
    info: dict[str, dict] = {}
    with tempfile.TemporaryDirectory() as d:
        srv = PodServer(Path(d) / "s.sock", device="cuda", lanes=2, memory_gb=60).start()
        try:
            clients = {}
            for name, t in TENANTS.items():
                progs, w = llama_decode_programs(m, PREFILL, t["max_len"], extend=(CHUNK,), window=t["window"])
                ps = PG.parse_variants(progs, w, gpu=True)
                need = (sum(p.bytes_estimate_for(srv.kernel_config) for p in ps)
                        - (len(ps) - 1) * (ps[0].param_bytes + ps[0].state_bytes))
                step = ps[1].compile("cuda", params=ps[0].tensors("cuda"), state=ps[0].state_tensors("cuda"))
                c = clients[name] = PodClient(srv.path, connect_timeout_s=120)
                rep = c.register(name, progs[0], w, memory_limit_gb=10, variants=progs[1:])
                info[name] = {"max_len": t["max_len"], "window": t["window"], "cache_slots": ps[1].state["kc0"].shape[1],
                              "loop_from_position": t["start"], "step_launches": step.stats["kernels"],
                              "ring_caches": step.stats["ring_caches"], "state_bytes": ps[0].state_bytes,
                              "cache_bytes": cache_bytes(ps[1]), "static_estimate_gb": round(need / 2 ** 30, 4),
                              "footprint_gb": rep["footprint_gb"]}
                del step
            torch.cuda.empty_cache()
            for r in range(a.warmup + a.runs):
                for name, t in TENANTS.items():
                    c = clients[name]
                    c.reset()
                    c.infer(ids[:, :PREFILL], outputs=[1])
                    for s in range(PREFILL, t["start"] - CHUNK, CHUNK):       # the extend chunks but the last
                        c.infer(ids[:, s:s + CHUNK], outputs=[1])
                    _, tm = c.generate(ids[:, t["start"] - CHUNK:t["start"]], a.tokens)   # the last chunk, then the loop
                    assert tm["state"]["pos"] == [t["start"] + a.tokens - 1], tm["state"]
                    if r >= a.warmup:
                        times[name].append(1e3 * tm["step_s"][0])
            for c in clients.values():
                c.close()
        finally:
            srv.stop()
    for name, v in times.items():
        info[name]["ms_per_token"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                                      "max": round(max(v), 4)}
    full, swa = info["full-8192"], info["swa-8192"]
    assert swa["cache_bytes"] * full["cache_slots"] == full["cache_bytes"] * swa["cache_slots"], (swa, full)
    res = {"what": "PodClient.generate's server loop, one 1024-hidden 8-layer vocab-32000 decoder alone: full caches at "
                   "max_len 8192, ring caches (window 1024) at max_len 8192, full caches at max_len 1024; ms per token "
                   "(the loop's wall time over its steps), the tenants alternating in one process",
           "tokens": a.tokens, "runs": a.runs, "warmup": a.warmup, "prefill": PREFILL, "chunk": CHUNK,
           "device": torch.cuda.get_device_name(0), "tenants": info,
           "swa_over_full_8192_ms": round(swa["ms_per_token"]["median"] / full["ms_per_token"]["median"], 4),
           "swa_over_full_1024_ms": round(swa["ms_per_token"]["median"] / info["full-1024"]["ms_per_token"]["median"], 4),
           "cache_bytes_ratio": round(swa["cache_bytes"] / full["cache_bytes"], 6),
           "cache_slots_over_max_len": round(swa["cache_slots"] / full["cache_slots"], 6)}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
