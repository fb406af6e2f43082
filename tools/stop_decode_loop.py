"""What stop ids and the repetition penalty cost a decode step.

One GPU pod server in this process, the fleet decoder (1024 hidden, 8 layers, 2 KV
heads of 128, vocab 32000, cache 1024) registered twice -- plain and with
``stopping=True`` -- and ``PodClient.generate``'s server loop run on one
configuration at a time, alternating:

1. ``plain``: the plain tenant;
2. ``stopping-unarmed``: the stopping tenant sent no ``stopping`` field (its three
   extra launches per step -- mark, penalise, stop step -- run on zero control words);
3. ``armed-W``: the stopping tenant with a repetition penalty of 1.3 and a stop id
   the run never draws (taken from a probe run: an id its tokens do not hold), so the
   loop runs every step and checks the rows' ``done`` flags every ``W`` steps, for
   ``W`` (``PodServer.stop_check_every``) in 4, 8, 16, 32.

Each run is a prefill plus ``--tokens`` - 1 decode steps in one request; its figure is
the loop's wall time over its steps.  Prints, and with ``--out`` writes, per
configuration ms per token (median, min, max over ``--runs``), the native launches of
each tenant's decode step and prefill (``launches``), what the step's three extra
launches cost against the plain tenant, and the default ``stop_check_every`` the numbers
support: the smallest W whose armed median lies within the run-to-run spread (max /
median) of the unarmed stopping tenant measured in the same run.

    python tools/stop_decode_loop.py --out profiles/stop_decode_loop.json
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

WINDOWS = (4, 8, 16, 32)
PENALTY = 1.3


def launches(m, a) -> dict:
    """The native launches of each tenant's two programs, compiled for the GPU: the decode step the
    loop replays (the stopping one: three more -- mark, penalise, stop step) and the prefill (one
    more still: its ``pos_set`` of ``done``)."""
    import torch

    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver import program as PG

    out = {}
    for name, kw in (("plain", {}), ("stopping", {"stopping": True})):
        ps = PG.parse_variants(*llama_decode_programs(m, a.prompt, a.max_len, **kw), gpu=True)
        params, state, derived = ps[0].tensors("cuda"), ps[0].state_tensors("cuda"), {}
        cs = [p.compile("cuda", params=params, state=state, derived=derived) for p in ps]
        out[name] = {which: {k: c.stats.get(k) for k in ("kernels", "stop_launches")}
                     for which, c in (("prefill", cs[0]), ("decode_step", cs[1]))}
        del ps, params, state, derived, cs
    torch.cuda.empty_cache()
    return out


def measure(m, a) -> dict:
    from nos_amd.models.llama_program import llama_decode_programs
    from nos_amd.podserver.client import PodClient
    from nos_amd.podserver.server import PodServer

    prompt = np.random.default_rng(0).integers(0, m.config.vocab_size, (1, a.prompt)).astype(np.int32)
    with tempfile.TemporaryDirectory() as d:
        srv = PodServer(Path(d) / "s.sock", device="cuda", lanes=2, memory_gb=60).start()
        try:
            clients = {}
            for name, kw in (("plain", {}), ("stopping", {"stopping": True})):
                progs, w = llama_decode_programs(m, a.prompt, a.max_len, **kw)
                c = clients[name] = PodClient(srv.path, connect_timeout_s=120)
                c.register(name, progs[0], w, memory_limit_gb=10, variants=progs[1:])
            # a stop id the armed run never draws: the loop then runs every step, checking as it goes
            probe, _ = clients["stopping"].generate(prompt, a.tokens, repetition_penalty=PENALTY)
            never = int(np.setdiff1d(np.arange(m.config.vocab_size), probe.reshape(-1))[0])
            armed = dict(eos_token_id=never, repetition_penalty=PENALTY)
            configs = {"plain": ("plain", {}, None), "stopping-unarmed": ("stopping", {}, None),
                       **{f"armed-{w}": ("stopping", armed, w) for w in WINDOWS}}
            times: dict[str, list[float]] = {k: [] for k in configs}
            for r in range(a.warmup + a.runs):
                for name, (tenant, kw, every) in configs.items():
                    if every is not None:
                        srv.stop_check_every = every
                    ids, tm = clients[tenant].generate(prompt, a.tokens, **kw)
                    if ids.shape[1] != a.tokens or tm["steps_run"] != a.tokens - 1:
                        raise SystemExit(f"{name}: the run ended early ({ids.shape}, {tm['steps_run']} steps)")
                    if r >= a.warmup:
                        times[name].append(1e3 * tm["step_s"][0])
            for c in clients.values():
                c.close()
        finally:
            srv.stop()
    ms = {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
          for k, v in times.items()}
    un = ms["stopping-unarmed"]
    spread = un["max"] / un["median"]
    within = [w for w in WINDOWS if ms[f"armed-{w}"]["median"] <= un["median"] * spread]
    return {"prompt": a.prompt, "max_len": a.max_len, "never_drawn_stop_id": never, "launches": launches(m, a),
            "ms_per_token": ms,
            "three_launches_cost_ms": round(un["median"] - ms["plain"]["median"], 4),
            "three_launches_cost_over_plain": round(un["median"] / ms["plain"]["median"], 4),
            "unarmed_spread_max_over_median": round(spread, 4),
            "armed_over_unarmed": {str(w): round(ms[f"armed-{w}"]["median"] / un["median"], 4) for w in WINDOWS},
            "default_rule": "the smallest W whose armed median <= unarmed median x (unarmed max / median)",
            "stop_check_every_supported": within[0] if within else None}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--prompt", type=int, default=16)
    ap.add_argument("--max-len", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("stop_decode_loop.py measures on the GPU: none found")
    from nos_amd.models.llama_program import llama_config, llama_model

    m = llama_model(llama_config(True), 0)
    res = {"what": "PodClient.generate's server loop, one 1024-hidden 8-layer vocab-32000 decoder alone: the plain tenant, "
                   "the stopping tenant unarmed, and armed (penalty 1.3, a stop id never drawn) at four check windows: "
                   "ms per token (the loop's wall time over its steps), the configurations alternating in one process",
           "tokens": a.tokens, "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           **measure(m, a)}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
