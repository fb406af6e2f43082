"""The decode step of the fleet-shaped Mixtral tenant with fp32, int8 and MXFP4 experts.

One GPU pod server in this process and three tenants of the same model
(``mixtral_config(False)``: 1024 hidden, 8 layers, 8 experts of 1408, top-2,
vocab 32000) with K / V caches of ``--max-len`` 1024 rows, registered with
``experts="fp32"``, ``"int8"`` and ``"mxfp4"``; everything but the expert
tensors is fp32 in all three.

``PodClient.generate``'s server loop runs on one tenant at a time, alternating.
Each run is a prefill plus ``--tokens`` - 1 decode steps in one request; its
figure is the loop's wall time over its steps.  Prints, and with ``--out``
writes:

* ms per token of each tenant (median, min, max over ``--runs``), each
  quantized tenant's ratio to the fp32-expert one, and the fp32-expert tenant's
  own run-to-run spread (max / median) to read the ratios against;
* each tenant's weight payload, static estimate and measured ``footprint_gb``;
* the expert bytes a decode step streams (top-k experts of every layer at
  their stored size) and the step's launch count with its ``moe_*`` statistics.

    python tools/moe_quant_decode_loop.py --out profiles/moe_quant_decode_loop.json
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
EXPERTS = ("fp32", "int8", "mxfp4")


def expert_bytes(fmt: str, H: int, I: int) -> int:
    """One expert's two tensors as stored: W13 [2I, H] and W2 [H, I] with their scales."""
    if fmt == "fp32":
        return 3 * H * I * 4
    if fmt == "int8":
        return 3 * H * I + (2 * I + H) * 4
    return 3 * H * I // 2 + 3 * H * I // 32


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
        raise SystemExit("moe_quant_decode_loop.py measures on the GPU: none found")
    from nos_amd.models.llama_program import llama_decode_programs, mixtral_config, mixtral_model
    from nos_amd.podserver import program as PG
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    model = mixtral_model(mixtral_config(False), 0)
    cfg = model.config
    prompt = np.random.default_rng(0).integers(0, 32000, (1, a.prompt)).astype(np.int32)
    times: dict[str, list[float]] = {fmt: [] for fmt in EXPERTS}
    info: dict[str, dict] = {}
    with tempfile.TemporaryDirectory() as d:
        srv = PodServer(Path(d) / "s.sock", device="cuda", lanes=2, memory_gb=40).start()
        try:
            clients = {}
            for fmt in EXPERTS:
                progs, w = llama_decode_programs(model, a.prompt, a.max_len, experts=fmt)
                ps = PG.parse_variants(progs, w, gpu=True)
                need = (sum(p.bytes_estimate_for(srv.kernel_config) for p in ps)
                        - (len(ps) - 1) * (ps[0].param_bytes + ps[0].state_bytes))
                step = ps[1].compile("cuda")   # the decode step's launch count, from a build of its own
                stats = {k: step.stats.get(k, 0) for k in MOE_STATS}
                del step
                torch.cuda.empty_cache()
                c = clients[fmt] = PodClient(srv.path, connect_timeout_s=60)
                rep = c.register("mixtral-" + fmt, progs[0], w, memory_limit_gb=8, variants=progs[1:])
                per = expert_bytes(fmt, cfg.hidden_size, cfg.intermediate_size)
                info[fmt] = {"payload_bytes": len(w),
                             "expert_payload_bytes": cfg.num_hidden_layers * cfg.num_local_experts * per,
                             "expert_bytes_per_token": cfg.num_hidden_layers * cfg.num_experts_per_tok * per,
                             "decode_step": stats, "static_estimate_gb": round(need / 2 ** 30, 4),
                             "footprint_gb": rep["footprint_gb"]}
            del model
            for r in range(a.warmup + a.runs):
                for fmt in EXPERTS:
                    _, tm = clients[fmt].generate(prompt, a.tokens)
                    if r >= a.warmup:
                        times[fmt].append(1e3 * tm["step_s"][0])
            for c in clients.values():
                c.close()
        finally:
            srv.stop()
    ms = {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
          for k, v in times.items()}
    base = ms["fp32"]
    res = {"what": "PodClient.generate's server loop, one tenant alone: the fleet-shaped Mixtral tenant (1024 hidden, 8 "
                   "layers, 8 experts of 1408, top-2, vocab 32000) registered with experts='fp32', 'int8' and 'mxfp4' "
                   "(everything but the expert tensors fp32), ms per token (the loop's wall time over its steps), "
                   "alternating in one process",
           "tokens": a.tokens, "prompt": a.prompt, "max_len": a.max_len, "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "ms_per_token": ms, "tenants": info,
           "fp32_spread_max_over_median": round(base["max"] / base["median"], 4),
           "over_fp32": {fmt: {"ratio": round(ms[fmt]["median"] / base["median"], 4),
                               "us_per_token": round(1e3 * (ms[fmt]["median"] - base["median"]), 2),
                               "expert_bytes_ratio": round(info[fmt]["expert_bytes_per_token"]
                                                           / info["fp32"]["expert_bytes_per_token"], 4)}
                         for fmt in EXPERTS if fmt != "fp32"}}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
