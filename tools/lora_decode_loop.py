"""The decode step of a multi-adapter LoRA decoder beside the plain one.

One GPU pod server in this process, the fleet decoder (1024 hidden, 8 layers,
vocab 32000, K / V caches of ``--max-len`` 1024 rows) registered as

* ``plain``: no adapters, fp32 weights;
* ``qv_r16``: 4 adapters of rank 16 on q + v;
* ``all7_r8``: 4 adapters of rank 8 on all seven projections;
* ``plain_int8`` and ``qv_r16_int8``: the first two with ``weights="int8"``,

and ``PodClient.generate``'s server loop run on one configuration at a time,
alternating: every adapter tenant with ``adapter`` 0 (the base model through
the adapter kernels) and 1.  Each run is a prefill plus ``--tokens`` - 1 decode
steps in one request; its figure is the loop's wall time over its steps.
Prints, and with ``--out`` writes:

* ms per token of each configuration (median, min, max over ``--runs``) and
  its ratio to the plain tenant of the same weights, measured in the same run;
* each tenant's decode-step launch count (``stats["kernels"]``) and its
  ``lora_shrinks``;
* each tenant's static estimate and measured ``footprint_gb``, and 4 x the
  plain tenant's: what four merged fine-tunes cost as four tenants.

    python tools/lora_decode_loop.py --out profiles/lora_decode_loop.json
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

QV = ("self_attn.q_proj", "self_attn.v_proj")
ALL7 = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
        "mlp.down_proj")


def random_adapters(model, n: int, targets, rank: int, seed: int = 1) -> list[dict]:
    rng = np.random.default_rng(seed)
    sd = model.state_dict()
    out = []
    for _ in range(n):
        ad = {}
        for i in range(model.config.num_hidden_layers):
            for t in targets:
                o, k = sd[f"model.layers.{i}.{t}.weight"].shape
                ad[f"model.layers.{i}.{t}"] = ((rng.standard_normal((rank, k)) / np.sqrt(k)).astype(np.float32),
                                               (0.02 * rng.standard_normal((o, rank))).astype(np.float32), 2.0)
        out.append(ad)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prompt", type=int, default=16)
    ap.add_argument("--max-len", type=int, default=1024)
    ap.add_argument("--adapters", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("lora_decode_loop.py measures on the GPU: none found")
    from nos_amd.models.llama_program import llama_config, llama_decode_programs, llama_model
    from nos_amd.podserver import program as PG
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    m = llama_model(llama_config(True), 0)
    prompt = np.random.default_rng(0).integers(0, m.config.vocab_size, (1, a.prompt)).astype(np.int32)
    qv, all7 = random_adapters(m, a.adapters, QV, 16), random_adapters(m, a.adapters, ALL7, 8)
    tenants = {"plain": ("fp32", None), "qv_r16": ("fp32", qv), "all7_r8": ("fp32", all7),
               "plain_int8": ("int8", None), "qv_r16_int8": ("int8", qv)}
    configs = [(name, ad) for name, (_, ads) in tenants.items() for ad in ((0, 1) if ads else (None,))]
    times: dict[str, list[float]] = {f"{n}/adapter={ad}" if ad is not None else n: [] for n, ad in configs}
    info: dict[str, dict] = {}
    with tempfile.TemporaryDirectory() as d:
        srv = PodServer(Path(d) / "s.sock", device="cuda", lanes=2, memory_gb=40).start()
        try:
            clients = {}
            for name, (weights, ads) in tenants.items():
                progs, w = llama_decode_programs(m, a.prompt, a.max_len, weights=weights, adapters=ads)
                ps = PG.parse_variants(progs, w, gpu=True)
                need = (sum(p.bytes_estimate_for(srv.kernel_config) for p in ps)
                        - (len(ps) - 1) * (ps[0].param_bytes + ps[0].state_bytes))
                step = ps[1].compile("cuda")   # the decode step's launch count, from a build of its own
                stats = {k: step.stats.get(k, 0) for k in ("kernels", "lora_shrinks", "lora_fused")}
                del step
                torch.cuda.empty_cache()
                c = clients[name] = PodClient(srv.path, connect_timeout_s=60)
                rep = c.register(name, progs[0], w, memory_limit_gb=8, variants=progs[1:])
                lora = sum(v.nbytes for k, v in ps[0].params.items() if ".lora_" in k)
                info[name] = {"payload_bytes": len(w), "adapter_bytes": lora, "decode_step": stats,
                              "static_estimate_gb": round(need / 2 ** 30, 4), "footprint_gb": rep["footprint_gb"]}
            for r in range(a.warmup + a.runs):
                for name, ad in configs:
                    _, tm = clients[name].generate(prompt, a.tokens, adapter=ad)
                    if r >= a.warmup:
                        times[f"{name}/adapter={ad}" if ad is not None else name].append(1e3 * tm["step_s"][0])
            for c in clients.values():
                c.close()
        finally:
            srv.stop()
    ms = {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
          for k, v in times.items()}
    for k, v in ms.items():
        v["over_plain"] = round(v["median"] / ms["plain_int8" if "int8" in k else "plain"]["median"], 4)
    res = {"what": "PodClient.generate's server loop, one 1024-hidden 8-layer vocab-32000 decoder alone: the plain "
                   "tenant and adapter tenants (4 LoRA adapters; adapter 0 = the base model through the adapter "
                   "kernels, adapter 1 = an adapter), ms per token (the loop's wall time over its steps), all "
                   "alternating in one process; over_plain: the ratio to the plain tenant of the same weights",
           "tokens": a.tokens, "prompt": a.prompt, "max_len": a.max_len, "runs": a.runs, "warmup": a.warmup,
           "adapters": a.adapters, "device": torch.cuda.get_device_name(0), "ms_per_token": ms, "tenants": info,
           "memory": {"one_adapter_tenant_gb": {"static_estimate": info["qv_r16"]["static_estimate_gb"],
                                                "footprint": info["qv_r16"]["footprint_gb"]},
                      "as_many_plain_tenants_gb": {"static_estimate": round(a.adapters * info["plain"]["static_estimate_gb"], 4),
                                                   "footprint": round(a.adapters * info["plain"]["footprint_gb"], 4)}}}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
