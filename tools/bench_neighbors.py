#!/usr/bin/env python3
"""Timing of the nearest-gene kernel (ops.knn_topk) on synthetic unit rows.

Per shape (Q queries x G genes x h, k = 10; default the ex shape
100 x 7523 x 128, the biomarker-query scale shape 100 x 1M x 512 and the
all-pairs scale shape 200k x 200k x 256) it prints one JSON line with

  knn_ms             device-event time of one knn_topk_ call (tile kernel +
                     merge kernel when the candidates are split), warmed,
                     median of --reps; knn_all_ms holds every repeat
  executed_tflops    2*Q*G*h / t, the FLOP the matrix unit executes (padded
                     rows of a partial query tile not counted)
  share_of_157TF     that over the 157 TF f32-MFMA peak
  stream_tbps        G*h*4 / t: X streamed once, against the 6.3 TB/s
                     streaming ceiling (meaningful where Q is small)
  torch_ms           the baseline: a (Xq_chunk @ X.T) -> self mask ->
                     .topk(k) loop over query chunks of at most --chunk-mb
                     of scores, same process, interleaved with the kernel
                     repeat by repeat; torch_reps of them
  idx_equal          share of result rows on which the baseline's indices
                     equal the kernel's (ties and last-bit differences of
                     another summation order may differ: not a gate)

Nothing here asserts a speed. Needs a GPU: without one it stops instead of
timing the CPU mirror."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from g2vec_amd import ops  # noqa: E402
from g2vec_amd.neighbors import unit_rows  # noqa: E402

MFMA_F32_PEAK = 157e12
STREAM_PEAK = 6.3e12
K = 10
SHAPES = {"ex": (100, 7523, 128), "1m": (100, 1_000_000, 512),
          "200k": (200_000, 200_000, 256)}


def timed(fn) -> float:
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_shape(name: str, Q: int, G: int, h: int, reps: int, torch_reps: int,
                chunk_mb: int, dev: torch.device, grid_y: int = 0) -> dict:
    gen = torch.Generator(device=dev).manual_seed(1)
    X = unit_rows(torch.randn(G, h, generator=gen, device=dev)).contiguous()
    qi = torch.randperm(G, generator=gen, device=dev)[:Q].int().contiguous()
    Xq = X[qi.long()].contiguous()
    nat = ops.native()
    gy = nat.knn_grid_y(Q, G, grid_y)
    idx = torch.empty(Q, K, dtype=torch.int32, device=dev)
    val = torch.empty(Q, K, dtype=torch.float32, device=dev)
    part_idx = part_val = None
    if gy > 1:
        part_idx = torch.empty(Q, gy, K, dtype=torch.int32, device=dev)
        part_val = torch.empty(Q, gy, K, dtype=torch.float32, device=dev)

    def run_knn():
        nat.knn_topk_(Xq, X, qi, K, grid_y, part_idx, part_val, idx, val)

    rows = max(1, min(Q, (chunk_mb << 20) // (4 * G)))
    t_idx = torch.empty(Q, K, dtype=torch.int64, device=dev)
    t_val = torch.empty(Q, K, dtype=torch.float32, device=dev)
    Xt = X.t()

    def run_torch():
        for lo in range(0, Q, rows):
            sc = Xq[lo:lo + rows] @ Xt
            n = sc.shape[0]
            sc[torch.arange(n, device=dev), qi[lo:lo + n].long()] = \
                float("-inf")
            v, i = sc.topk(K, dim=1)
            t_val[lo:lo + n] = v
            t_idx[lo:lo + n] = i

    for _ in range(2):                               # warm both
        run_knn()
        run_torch()
    torch.cuda.synchronize()
    t_knn, t_torch = [], []
    for r in range(reps):                            # interleaved
        t_knn.append(timed(run_knn))
        if r < torch_reps:
            t_torch.append(timed(run_torch))
    med = statistics.median(t_knn) * 1e-3
    med_t = statistics.median(t_torch) * 1e-3
    flop = 2.0 * Q * G * h
    return {
        "shape": name, "Q": Q, "G": G, "h": h, "k": K, "grid_y": int(gy),
        "reps": reps, "device": torch.cuda.get_device_name(0),
        "knn_ms": round(med * 1e3, 4),
        "knn_all_ms": [round(t, 4) for t in t_knn],
        "executed_tflops": round(flop / med / 1e12, 3),
        "share_of_157TF": round(flop / med / MFMA_F32_PEAK, 4),
        "stream_tbps": round(G * h * 4.0 / med / 1e12, 4),
        "share_of_6.3TBps": round(G * h * 4.0 / med / STREAM_PEAK, 4),
        "torch_ms": round(med_t * 1e3, 4),
        "torch_all_ms": [round(t, 4) for t in t_torch],
        "torch_reps": len(t_torch), "torch_chunk_rows": rows,
        "torch_over_knn": round(med_t / med, 3),
        "idx_equal": round(float((t_idx.int() == idx).all(dim=1)
                                 .float().mean()), 5),
        "max_abs_val_diff": float((t_val - val).abs().max()),
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="ex,1m,200k",
                    help="comma list of " + "/".join(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=0,
                    help="baseline repeats (default: --reps, 3 at 200k)")
    ap.add_argument("--chunk-mb", type=int, default=1024,
                    help="score bytes per baseline query chunk")
    ap.add_argument("--grid-y", type=int, default=0,
                    help="force the kernel's candidate split (0 = automatic)")
    ap.add_argument("--out-prefix", default="",
                    help="also write PREFIX<shape>.json per shape")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_neighbors needs a GPU: nothing measured", file=sys.stderr)
        return 2
    for name in args.shapes.split(","):
        Q, G, h = SHAPES[name]
        t_reps = args.torch_reps or (3 if name == "200k" else args.reps)
        rec = bench_shape(name, Q, G, h, args.reps, t_reps, args.chunk_mb,
                          torch.device("cuda", 0), args.grid_y)
        print(json.dumps(rec), flush=True)
        if args.out_prefix:
            with open(f"{args.out_prefix}{name}.json", "w") as fh:
                fh.write(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
