"""The decode step of a mixture-of-experts decoder beside the dense one.

One GPU pod server in this process and two tenants with K / V caches of
``--max-len`` 1024 rows:

* ``dense``: the fleet decoder (1024 hidden, 8 layers, MLP 2816, vocab 32000);
* ``mixtral``: the fleet-shaped Mixtral tenant (``mixtral_config(False)``: the
  same attention half, the MLP as E = 8 experts of 1408 with k = 2, so a token
  streams the dense decoder's MLP bytes plus the router's).

``PodClient.generate``'s server loop runs on one tenant at a time, alternating.
Each run is a prefill plus ``--tokens`` - 1 decode steps in one request; its
figure is the loop's wall time over its steps.  Prints, and with ``--out``
writes:

* ms per token of each tenant (median, min, max over ``--runs``) and the
  Mixtral tenant's ratio to and difference from the dense one, with the
  difference per added launch;
* each tenant's decode-step launch count (``stats["kernels"]``) and the
  Mixtral step's ``moe_*`` statistics;
* each tenant's weight payload, static estimate and measured ``footprint_gb``.

    python tools/moe_decode_loop.py --out profiles/moe_decode_loop.json
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

MOE_STATS = ("kernels", "moe_blocks", "moe_launches", "moe_rms_prologue", "moe_residual_fused")


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
        raise SystemExit("moe_decode_loop.py measures on the GPU: none found")
    from nos_amd.models.llama_program import (llama_config, llama_decode_programs, llama_model, mixtral_config,
                                              mixtral_model)
    from nos_amd.podserver import program as PG
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    models = {"dense": llama_model(llama_config(True), 0), "mixtral": mixtral_model(mixtral_config(False), 0)}
    prompt = np.random.default_rng(0).integers(0, 32000, (1, a.prompt)).astype(np.int32)
    times: dict[str, list[float]] = {name: [] for name in models}
    info: dict[str, dict] = {}
    with tempfile.TemporaryDirectory() as d:
        srv = PodServer(Path(d) / "s.sock", device="cuda", lanes=2, memory_gb=40).start()
        try:
            clients = {}
            for name, m in models.items():
                progs, w = llama_decode_programs(m, a.prompt, a.max_len)
                ps = PG.parse_variants(progs, w, gpu=True)
                need = (sum(p.bytes_estimate_for(srv.kernel_config) for p in ps)
                        - (len(ps) - 1) * (ps[0].param_bytes + ps[0].state_bytes))
                step = ps[1].compile("cuda")   # the decode step's launch count, from a build of its own
                stats = {k: step.stats.get(k, 0) for k in MOE_STATS}
                del step
                torch.cuda.empty_cache()
                c = clients[name] = PodClient(srv.path, connect_timeout_s=60)
                rep = c.register(name, progs[0], w, memory_limit_gb=8, variants=progs[1:])
                info[name] = {"payload_bytes": len(w), "decode_step": stats,
                              "static_estimate_gb": round(need / 2 ** 30, 4), "footprint_gb": rep["footprint_gb"]}
            models.clear()
            for r in range(a.warmup + a.runs):
                for name in clients:
                    _, tm = clients[name].generate(prompt, a.tokens)
                    if r >= a.warmup:
                        times[name].append(1e3 * tm["step_s"][0])
            for c in clients.values():
                c.close()
        finally:
            srv.stop()
    ms = {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
          for k, v in times.items()}
    added = info["mixtral"]["decode_step"]["kernels"] - info["dense"]["decode_step"]["kernels"]
    delta_us = 1e3 * (ms["mixtral"]["median"] - ms["dense"]["median"])
    res = {"what": "PodClient.generate's server loop, one decoder alone: the dense fleet decoder (1024 hidden, 8 layers, "
                   "MLP 2816, vocab 32000) and the fleet-shaped Mixtral tenant (the same attention, the MLP as 8 experts "
                   "of 1408, top-2), ms per token (the loop's wall time over its steps), alternating in one process",
           "tokens": a.tokens, "prompt": a.prompt, "max_len": a.max_len, "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "ms_per_token": ms, "tenants": info,
           "mixtral_over_dense": {"ratio": round(ms["mixtral"]["median"] / ms["dense"]["median"], 4),
                                  "added_us_per_token": round(delta_us, 2), "added_launches": added,
                                  "us_per_added_launch": round(delta_us / added, 2) if added else None}}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
