#!/usr/bin/env python3
"""Timing of the permutation-null kernels (ops.perm_t_counts, and the
col_moments pass it needs once per run) on synthetic centred expression.

Per shape (G genes, S samples, B relabellings; default the ex shape
7.5k x 135 x 10k and the scale shapes 200k x 300 x 1k and 1M x 300 x 1k) it
prints one JSON line with

  counts_ms          device-event time of one perm_t_counts launch over all
                     B relabellings (two memsets + the kernel), warmed,
                     median of --reps; counts_all_ms holds every repeat
  tflops             8*G*S*B / t. Convention: the kernel runs two GEMMs
                     (s1 and q1) of 2*G*S*B FLOP each = 4*G*S*B executed on
                     the matrix unit; the figure counts twice that because
                     the second label group's sums are derived (T - s1,
                     Q - q1) instead of computed. executed_tflops is the
                     4*G*S*B figure.
  share_of_157TF     executed_tflops over the 157 TF f32-MFMA peak (the
                     derived half is not matrix work)
  moments_ms         device-event time of col_moments
  host_loop          ex shape only: seconds of 20 scoring.t_scores calls on
                     relabelled data, the per-relabelling mean, that mean
                     times B (EXTRAPOLATED, not run), and its ratio to the
                     kernel time

Nothing here asserts a speed. Needs a GPU: without one it stops instead of
timing the CPU mirrors."""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from g2vec_amd import ops, scoring  # noqa: E402

MFMA_F32_PEAK = 157e12
SHAPES = {"ex": (7523, 135, 10_000), "200k": (200_000, 300, 1000),
          "1m": (1_000_000, 300, 1000)}


def event_ms(fn, reps: int, warm: int = 3):
    times = []
    for i in range(reps + warm):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            times.append(a.elapsed_time(b))
    return times


def bench_shape(name: str, G: int, S: int, B: int, reps: int,
                dev: torch.device) -> dict:
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(S, G, generator=gen)
    x = (x.double() - x.double().mean(dim=0)).float().contiguous()
    labels = (np.arange(S) % 5 < 2).astype(np.int64)
    n1 = int(labels.sum())
    expr = x.to(dev)
    masks = torch.from_numpy(scoring.perm_masks(labels, B, seed=0)).to(dev)
    obs = torch.from_numpy(labels.astype(np.uint8)[None, :]).to(dev)
    stat_obs = ops.perm_t_stats(expr, obs)[0].contiguous()
    T, Q = ops.col_moments(expr)
    counts = torch.empty(G, dtype=torch.int32, device=dev)
    maxstat = torch.empty(B, dtype=torch.float64, device=dev)
    nat = ops.native()

    def run_counts():
        nat.perm_t_counts_(expr, masks, T, Q, n1, stat_obs, counts, maxstat)

    def run_moments():
        nat.col_moments_(expr, T, Q)

    t_counts = event_ms(run_counts, reps)
    t_mom = event_ms(run_moments, reps)
    med = statistics.median(t_counts) * 1e-3
    rec = {
        "shape": name, "G": G, "S": S, "B": B, "reps": reps,
        "device": torch.cuda.get_device_name(0),
        "counts_ms": round(med * 1e3, 4),
        "counts_all_ms": [round(t, 4) for t in t_counts],
        "flop_convention": "tflops = 8*G*S*B/t (two GEMMs of 2*G*S*B, both "
                           "label groups); executed = 4*G*S*B/t",
        "tflops": round(8.0 * G * S * B / med / 1e12, 3),
        "executed_tflops": round(4.0 * G * S * B / med / 1e12, 3),
        "share_of_157TF": round(4.0 * G * S * B / med / MFMA_F32_PEAK, 4),
        "moments_ms": round(statistics.median(t_mom), 4),
        "genes_at_min_p": int((counts == 0).sum()),
    }
    if name == "ex":
        x_np = x.numpy()
        m_np = masks[:20].cpu().numpy()
        scoring.t_scores(x_np, labels)                     # warm
        t0 = time.perf_counter()
        for b in range(20):
            scoring.t_scores(x_np, m_np[b].astype(np.int64))
        dt = time.perf_counter() - t0
        rec["host_loop"] = {
            "relabellings_run": 20, "seconds": round(dt, 4),
            "seconds_per_relabelling": round(dt / 20, 5),
            "extrapolated_seconds_at_B": round(dt / 20 * B, 2),
            "extrapolated_ratio_to_kernel": round(dt / 20 * B / med, 1),
            "note": "EXTRAPOLATED from 20 relabellings to B; the host loop "
                    "was not run at B",
        }
    return rec


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="ex,200k,1m",
                    help="comma list of " + "/".join(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out-prefix", default="",
                    help="also write PREFIX<shape>.json per shape")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_perm needs a GPU: nothing measured", file=sys.stderr)
        return 2
    for name in args.shapes.split(","):
        G, S, B = SHAPES[name]
        rec = bench_shape(name, G, S, B, args.reps, torch.device("cuda", 0))
        print(json.dumps(rec), flush=True)
        if args.out_prefix:
            with open(f"{args.out_prefix}{name}.json", "w") as fh:
                fh.write(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
