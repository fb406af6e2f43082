"""Forward + backward of a training tenant's attention, chunked against flash
(podserver/train_ops.py), timed with device events in one process.

python tools/attn_train_bench.py --seq 2048 [--batch 1 --heads 8 --kv-heads 2 --head-dim 128 --reps 5]

The two paths alternate (chunked, flash, chunked, ...) after a warm-up of
each, so clock and thermal drift hit both alike.  Prints one JSON line: the
per-repetition times, their median and spread (max - min), the FLOPs the
algorithm needs and the resulting useful-work rate.

FLOPs, by the formula kept here: the forward is two S x S x D products
(Q K^T, P V) = 4 B H Sq Skv D, the backward five (recomputed S is not
counted: it is the implementation's choice) = 10 B H Sq Skv D; a causal mask
halves both.  The rate is useful work over time, not a share of the chip's
peak -- fp32-class results on fp16x3 pipes cost three MFMAs per product.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def attention_flops(b: int, h: int, sq: int, skv: int, d: int, causal: bool) -> dict:
    fwd, bwd = 4 * b * h * sq * skv * d, 10 * b * h * sq * skv * d
    if causal:
        fwd, bwd = fwd // 2, bwd // 2
    return {"forward": fwd, "backward": bwd, "total": fwd + bwd}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--kv-heads", type=int, default=2)
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--causal", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        print("attn_train_bench: no GPU", file=sys.stderr)
        return 1
    from nos_amd.podserver import train_ops

    B, S, H, Hkv, D, causal = a.batch, a.seq, a.heads, a.kv_heads, a.head_dim, bool(a.causal)
    g = torch.Generator(device="cuda").manual_seed(0)
    # q / k / v as a training step sees them: slices of one fused projection
    qkv = torch.randn(B, S, (H + 2 * Hkv) * D, device="cuda", generator=g)
    q = qkv[..., :H * D].view(B, S, H, D).requires_grad_()
    k = qkv[..., H * D:(H + Hkv) * D].view(B, S, Hkv, D).requires_grad_()
    v = qkv[..., (H + Hkv) * D:].view(B, S, Hkv, D).requires_grad_()
    do = torch.randn(B, S, H, D, device="cuda", generator=g)
    paths = {"chunked": train_ops.attention, "flash": train_ops.flash_attention}

    def once(fn) -> float:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        o = fn(q, k, v, causal)
        torch.autograd.grad(o, (q, k, v), do)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    for fn in paths.values():
        for _ in range(a.warmup):
            once(fn)
    times: dict[str, list[float]] = {n: [] for n in paths}
    for _ in range(a.reps):
        for n, fn in paths.items():
            times[n].append(once(fn))
    fl = attention_flops(B, H, S, S, D, causal)
    out = {"shape": {"B": B, "S": S, "H": H, "Hkv": Hkv, "D": D, "causal": causal}, "reps": a.reps, "flops": fl}
    for n, ts in times.items():
        med = statistics.median(ts)
        out[n] = {"ms": [round(t, 3) for t in ts], "median_ms": round(med, 3), "spread_ms": round(max(ts) - min(ts), 3),
                  "useful_tflops": round(fl["total"] / (med * 1e-3) / 1e12, 2)}
    out["speedup"] = round(out["chunked"]["median_ms"] / out["flash"]["median_ms"], 2)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
