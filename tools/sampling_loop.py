"""Cost of the sampled decode step in the pod server's generate loop.

One GPU pod server in this process, the fleet decoder (1024 hidden, 8 layers,
fp32, vocab 32000) registered twice -- with ``argmax`` programs (the baseline)
and with ``sample`` programs -- and ``PodClient.generate``'s server loop run
on one of them at a time, the modes alternating:

* ``greedy``        the argmax tenant;
* ``sample_greedy`` the sampling tenant without parameters (ctl zeros);
* ``temperature``   temperature 0.8 alone;
* ``top_k_top_p``   temperature 0.8, top_k 50, top_p 0.9.

Each run is a prefill plus ``--tokens`` - 1 decode steps in one request; its
figure is the loop's wall time over its steps (the request ends in the
lane's synchronise).  Prints, and with ``--out`` writes, the per-mode ms per
token (median, min, max over ``--runs``) and the ratios to ``greedy``.

    python tools/sampling_loop.py --out profiles/sampled_generate_loop.json
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

MODES = {"greedy": None, "sample_greedy": {}, "temperature": {"temperature": 0.8},
         "top_k_top_p": {"temperature": 0.8, "top_k": 50, "top_p": 0.9}}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prompt", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("sampling_loop.py measures on the GPU: none found")
    from nos_amd.models.llama_program import llama_config, llama_decode_programs, llama_model
    from nos_amd.ops import _lib
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    m = llama_model(llama_config(True), 0)
    max_len = 1 << (a.prompt + a.tokens).bit_length()
    prompt = np.random.default_rng(0).integers(0, m.config.vocab_size, (1, a.prompt)).astype(np.int32)
    times: dict[str, list[float]] = {k: [] for k in MODES}
    ids = {}
    with tempfile.TemporaryDirectory() as d:
        srv = PodServer(Path(d) / "s.sock", device="cuda", lanes=2, memory_gb=40).start()
        try:
            clients = {}
            for name, sampling in (("argmax", False), ("sample", True)):
                progs, w = llama_decode_programs(m, a.prompt, max_len, sampling=sampling)
                c = clients[name] = PodClient(srv.path, connect_timeout_s=60)
                c.register(name, progs[0], w, memory_limit_gb=8, variants=progs[1:])
            for r in range(a.warmup + a.runs):
                for mode, kw in MODES.items():
                    c = clients["argmax" if kw is None else "sample"]
                    out, tm = c.generate(prompt, a.tokens, seed=r if kw else 0, **(kw or {}))
                    if r >= a.warmup:
                        times[mode].append(1e3 * tm["step_s"][0])
                    ids[mode] = out
            for c in clients.values():
                c.close()
        finally:
            srv.stop()
    if not np.array_equal(ids["greedy"], ids["sample_greedy"]):
        raise SystemExit("the sampling tenant without parameters is not greedy")
    res = {"what": "PodClient.generate's server loop, one fp32 1024-hidden 8-layer vocab-32000 decoder alone: ms per "
                   "token (the loop's wall time over its steps), modes alternating in one process",
           "tokens": a.tokens, "prompt": a.prompt, "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0),
           "row_in_lds": bool(_lib.lib().nos_sample_row_in_lds(m.config.vocab_size)),
           "ms_per_token": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                                "max": round(max(v), 4)} for k, v in times.items()}}
    base = res["ms_per_token"]["greedy"]["median"]
    res["ratio_to_greedy"] = {k: round(v["median"] / base, 4) for k, v in res["ms_per_token"].items()}
    res["distinct_tokens"] = {k: int(len(set(v.reshape(-1).tolist()))) for k, v in ids.items()}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
