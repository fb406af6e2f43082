"""Speculative decoding (n-gram drafts, device verify) beside the plain decode loop.

One GPU pod server in this process, the fleet decoder (1024 hidden, 8 layers,
vocab 32000, K / V caches of ``--max-len`` 1024 rows) registered plain and
with ``speculate=4`` and ``speculate=8``, and ``PodClient.generate``'s server
loop run on one of them at a time, alternating, on two prompts: 16 tokens of
period 4, and 16 random ids.  Each run is a prefill plus one ``generate``
request for ``--tokens`` - 1 more tokens; the figures are of that request
alone.  Prints, and with ``--out`` writes, per configuration and prompt:

* ms per token: the loop's wall time over the tokens it produced (median, min,
  max over ``--runs``);
* tokens per step: the mean of ``n_acc`` over the verify steps the server ran
  (the steps a check window overran, which advance by 0, included);
* ms per verify step: the loop's wall time over ``steps_run``;

and the headline values: the verify step's time over the plain step's, and
each speculating tenant's ms per token over the plain tenant's.

    python tools/spec_decode_loop.py --out profiles/spec_decode_loop.json
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
        raise SystemExit("spec_decode_loop.py measures on the GPU: none found")
    from nos_amd.models.llama_program import llama_config, llama_decode_programs, llama_model
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    m = llama_model(llama_config(True), 0)
    rng = np.random.default_rng(0)
    prompts = {"periodic": np.tile(rng.integers(0, m.config.vocab_size, 4), a.prompt // 4 + 1)[None, :a.prompt],
               "random": rng.integers(0, m.config.vocab_size, (1, a.prompt))}
    prompts = {k: v.astype(np.int32) for k, v in prompts.items()}
    configs = {"plain": None, "speculate4": 4, "speculate8": 8}
    runs = {(c, p): [] for c in configs for p in prompts}    # (ms per token, ms per step, tokens per step, steps_run)
    tokens, info = {}, {}
    with tempfile.TemporaryDirectory() as d:
        srv = PodServer(Path(d) / "s.sock", device="cuda", lanes=2, memory_gb=40).start()
        try:
            clients = {}
            for name, k in configs.items():
                progs, w = llama_decode_programs(m, a.prompt, a.max_len, speculate=k)
                c = clients[name] = PodClient(srv.path, connect_timeout_s=60)
                rep = c.register(name, progs[0], w, memory_limit_gb=8, variants=progs[1:])
                info[name] = {"footprint_gb": rep["footprint_gb"], "variants": rep["input_shapes"]}
            for r in range(a.warmup + a.runs):
                for pn, prompt in prompts.items():
                    for name, k in configs.items():
                        ids, tm = clients[name].generate(prompt, a.tokens, speculate=k is not None)
                        run = tm["steps_run"]
                        loop_ms = 1e3 * tm["step_s"][0] * run
                        tokens.setdefault(pn, {})[name] = ids
                        if r >= a.warmup:
                            acc = tm["n_acc"] if k else np.ones((run, 1))
                            runs[(name, pn)].append((loop_ms / (a.tokens - 1), loop_ms / run, float(acc.mean()), run))
            for c in clients.values():
                c.close()
        finally:
            srv.stop()

    def stat(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    res = {"what": "PodClient.generate's server loop on one 1024-hidden 8-layer vocab-32000 decoder alone, registered "
                   "plain and with speculate=4 and 8, the three alternating in one process on a periodic and a random "
                   "16-token prompt: the generate request's wall time per token and per step",
           "tokens": a.tokens, "prompt": a.prompt, "max_len": a.max_len, "runs": a.runs, "warmup": a.warmup,
           "stop_check_every": srv.stop_check_every, "device": torch.cuda.get_device_name(0), "tenants": info,
           "results": {}}
    for pn in prompts:
        plain = stat([v[0] for v in runs[("plain", pn)]])["median"]
        for name in configs:
            v = runs[(name, pn)]
            ent = {"ms_per_token": stat([x[0] for x in v]), "ms_per_step": stat([x[1] for x in v]),
                   "tokens_per_step": round(statistics.median([x[2] for x in v]), 4),
                   "steps_run": int(statistics.median([x[3] for x in v])),
                   "tokens_equal_plain": bool(np.array_equal(tokens[pn][name], tokens[pn]["plain"]))}
            ent["step_over_plain_step"] = round(ent["ms_per_step"]["median"] / plain, 4)
            ent["ms_per_token_over_plain"] = round(ent["ms_per_token"]["median"] / plain, 4)
            res["results"].setdefault(pn, {})[name] = ent
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
