#!/usr/bin/env python3
"""Timing of the silhouette kernel (ops.cluster_dist_sums) on synthetic
Gaussian rows with random labels.

Per shape (Q queries x G genes x h, k = 3; default the ex all-pairs shape
7523 x 7523 x 128, the biomarker-query scale shape 100 x 1M x 512 and the
all-pairs scale shape 200k x 200k x 256) it prints one JSON line with

  cds_ms             device-event time of one cluster_dist_sums_ call (the
                     two squared-norm launches, the tile kernel and the fold
                     when the candidates are split) at the op's automatic
                     split, warmed, median of --reps (3 at 200k); cds_all_ms
                     holds every repeat
  cds_sil_ms         the same at the split cluster_quality.silhouette asks
                     for (a function of G alone), grid_y_sil
  executed_tflops    2*Q*G*h / t, the FLOP the matrix unit executes
  share_of_157TF     that over the 157 TF f32-MFMA peak
  cdist_ms           baseline 1: torch.cdist(Xq_chunk, X) -> self mask -> one
                     masked f64 row sum per cluster, over query chunks of at
                     most --chunk-mb of distances
  knn_ms             baseline 2: ops.knn_topk at k = 10 on the same operands;
                     the same product, so knn_ms / cds_ms isolates the
                     epilogue
  max_rel_diff       largest relative difference between the kernel's D and
                     baseline 1's (another formula and summation order: not a
                     gate)

The three run in one process, interleaved repeat by repeat. Nothing here
asserts a speed. Needs a GPU: without one it stops instead of timing the CPU
mirror."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from g2vec_amd import ops  # noqa: E402
from g2vec_amd.cluster_quality import sil_grid_y  # noqa: E402

MFMA_F32_PEAK = 157e12
K = 3
KNN_K = 10
SHAPES = {"ex": (7523, 7523, 128), "1m": (100, 1_000_000, 512),
          "200k": (200_000, 200_000, 256)}


def timed(fn) -> float:
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_shape(name: str, Q: int, G: int, h: int, reps: int, chunk_mb: int,
                dev: torch.device, grid_y: int = 0) -> dict:
    gen = torch.Generator(device=dev).manual_seed(1)
    X = torch.randn(G, h, generator=gen, device=dev)
    X = (X - X.mean(dim=0)).contiguous()
    labels = torch.randint(0, K, (G,), generator=gen, device=dev).int()
    qi = torch.randperm(G, generator=gen, device=dev)[:Q].int().contiguous()
    Xq = X[qi.long()].contiguous()
    nat = ops.native()
    nq = torch.empty(Q, dtype=torch.float32, device=dev)
    nx = torch.empty(G, dtype=torch.float32, device=dev)

    def cds_runner(gy_arg):
        gy = nat.cds_grid_y(Q, G, K, gy_arg)
        D = torch.empty(Q, K, dtype=torch.float64, device=dev)
        part = None
        if gy > 1:
            part = torch.empty(Q, gy, K, dtype=torch.float64, device=dev)
        return gy, D, lambda: nat.cluster_dist_sums_(
            Xq, X, labels, qi, K, gy_arg, nq, nx, part, D)

    gy, D, run_cds = cds_runner(grid_y)
    gy_sil, D_sil, run_sil = cds_runner(sil_grid_y(G))

    kgy = nat.knn_grid_y(Q, G, 0)
    idx = torch.empty(Q, KNN_K, dtype=torch.int32, device=dev)
    val = torch.empty(Q, KNN_K, dtype=torch.float32, device=dev)
    part_idx = part_val = None
    if kgy > 1:
        part_idx = torch.empty(Q, kgy, KNN_K, dtype=torch.int32, device=dev)
        part_val = torch.empty(Q, kgy, KNN_K, dtype=torch.float32, device=dev)

    def run_knn():
        nat.knn_topk_(Xq, X, qi, KNN_K, 0, part_idx, part_val, idx, val)

    rows = max(1, min(Q, (chunk_mb << 20) // (4 * G)))
    t_D = torch.empty(Q, K, dtype=torch.float64, device=dev)
    masks = [labels == c for c in range(K)]

    def run_cdist():
        for lo in range(0, Q, rows):
            d = torch.cdist(Xq[lo:lo + rows], X)
            n = d.shape[0]
            d[torch.arange(n, device=dev), qi[lo:lo + n].long()] = 0.0
            for c in range(K):
                t_D[lo:lo + n, c] = torch.where(masks[c], d, 0.0).sum(
                    dim=1, dtype=torch.float64)

    for _ in range(2):                               # warm all
        run_cds()
        run_sil()
        run_knn()
        run_cdist()
    torch.cuda.synchronize()
    t_cds, t_sil, t_knn, t_cdist = [], [], [], []
    for _ in range(reps):                            # interleaved
        t_cds.append(timed(run_cds))
        t_sil.append(timed(run_sil))
        t_knn.append(timed(run_knn))
        t_cdist.append(timed(run_cdist))
    med = statistics.median(t_cds) * 1e-3
    med_s = statistics.median(t_sil) * 1e-3
    med_k = statistics.median(t_knn) * 1e-3
    med_c = statistics.median(t_cdist) * 1e-3
    flop = 2.0 * Q * G * h
    return {
        "shape": name, "Q": Q, "G": G, "h": h, "k": K, "grid_y": int(gy),
        "grid_y_sil": int(gy_sil), "knn_grid_y": int(kgy), "reps": reps,
        "device": torch.cuda.get_device_name(0),
        "cds_ms": round(med * 1e3, 4),
        "cds_all_ms": [round(t, 4) for t in t_cds],
        "cds_sil_ms": round(med_s * 1e3, 4),
        "cds_sil_all_ms": [round(t, 4) for t in t_sil],
        "executed_tflops": round(flop / med / 1e12, 3),
        "share_of_157TF": round(flop / med / MFMA_F32_PEAK, 4),
        "executed_tflops_sil": round(flop / med_s / 1e12, 3),
        "knn_ms": round(med_k * 1e3, 4),
        "knn_all_ms": [round(t, 4) for t in t_knn],
        "knn_over_cds": round(med_k / med, 3),
        "cdist_ms": round(med_c * 1e3, 4),
        "cdist_all_ms": [round(t, 4) for t in t_cdist],
        "cdist_chunk_rows": rows,
        "cdist_over_cds": round(med_c / med, 3),
        "max_rel_diff": float(((t_D - D).abs() / t_D).max()),
        "max_rel_diff_splits": float(((D_sil - D).abs() / D).max()),
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="ex,1m,200k",
                    help="comma list of " + "/".join(SHAPES))
    ap.add_argument("--reps", type=int, default=0,
                    help="repeats (default: 20, 3 at 200k)")
    ap.add_argument("--chunk-mb", type=int, default=1024,
                    help="distance bytes per baseline query chunk")
    ap.add_argument("--grid-y", type=int, default=0,
                    help="force the kernel's candidate split (0 = automatic)")
    ap.add_argument("--out-prefix", default="",
                    help="also write PREFIX<shape>.json per shape")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_silhouette needs a GPU: nothing measured",
              file=sys.stderr)
        return 2
    for name in args.shapes.split(","):
        Q, G, h = SHAPES[name]
        reps = args.reps or (3 if name == "200k" else 20)
        rec = bench_shape(name, Q, G, h, reps, args.chunk_mb,
                          torch.device("cuda", 0), args.grid_y)
        print(json.dumps(rec), flush=True)
        if args.out_prefix:
            with open(f"{args.out_prefix}{name}.json", "w") as fh:
                fh.write(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
