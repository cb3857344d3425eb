#!/usr/bin/env python3
"""Timing of the rank kernels (ops.rank_columns, ops.ranksum_scores) on
synthetic expression.

Per shape (S samples x G genes; default 68 x 7523, the ex shape 135 x 7523
and the scale shapes 300 x 200k and 300 x 1M) it prints one JSON line with

  rank_ms / ranksum_ms   device-event time of one launch, warmed, median of
                         --reps; *_all_ms holds every repeat
  pairs_per_s            S*S*G pair tests over the median time
  share_of_valu_ceiling  4 VALU lane-operations per pair test over a chip
                         ceiling of 3.9e13 lane-operations/s (256 CUs x 64
                         lanes x 2.4 GHz). A DERIVED yardstick, not a
                         measured peak.
  argsort2_ms            X.argsort(0).argsort(0) in the same process,
                         interleaved with the kernels repeat by repeat. It
                         does LESS work: ordinal ranks, ties ignored, two
                         int64 [S, G] temporaries.
  ratio_to_argsort2      argsort2_ms / rank_ms

--phase additionally times steps 2b-3 (pipeline.generate_paths) on an
ex-shaped synthetic data set with corr = pearson and spearman: each is run
PHASE_WARM + PHASE_REPS times, interleaved run by run, and the warmed runs are
reported (median, min, max) as the graphs_walks_overlapped phase (host time of
the enqueue, as the pipeline's timers see it) and as the synchronized wall
time of the whole call.

Nothing here asserts a speed. Needs a GPU: without one it stops instead of
timing the CPU mirrors."""
import argparse
import json
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from g2vec_amd import ops  # noqa: E402

VALU_LANE_OPS = 256 * 64 * 2.4e9        # derived chip ceiling, lane-ops/s
OPS_PER_PAIR = 4.0                      # 2 compares + 2 conditional adds
PHASE_WARM, PHASE_REPS = 2, 7         # --phase: interleaved runs per corr
SHAPES = {"ex68": (68, 7523), "ex": (135, 7523), "200k": (300, 200_000),
          "1m": (300, 1_000_000)}


def timed(fn) -> float:
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ts):
    return {"median": round(statistics.median(ts), 4),
            "min": round(min(ts), 4), "max": round(max(ts), 4)}


def bench_shape(name: str, S: int, G: int, reps: int, warm: int,
                dev: torch.device) -> dict:
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(S, G, generator=gen).to(dev)
    labels = torch.from_numpy((np.arange(S) % 5 < 2).astype(np.int32)).to(dev)
    nat = ops.native()
    ranks = torch.empty_like(x)
    z = torch.empty(G, dtype=torch.float32, device=dev)
    auc = torch.empty(G, dtype=torch.float32, device=dev)
    runs = {
        "rank": lambda: nat.rank_columns_(x, ranks),
        "ranksum": lambda: nat.ranksum_scores_(x, labels, z, auc),
        "argsort2": lambda: x.argsort(0).argsort(0),
    }
    times = {k: [] for k in runs}
    for i in range(reps + warm):            # interleaved repeat by repeat
        for k, fn in runs.items():
            t = timed(fn)
            if i >= warm:
                times[k].append(t)
    pairs = float(S) * S * G
    rec = {"shape": name, "S": S, "G": G, "reps": reps,
           "device": torch.cuda.get_device_name(0),
           "valu_ceiling_lane_ops_per_s": VALU_LANE_OPS,
           "lane_ops_per_pair": OPS_PER_PAIR}
    for k in ("rank", "ranksum"):
        med = statistics.median(times[k]) * 1e-3
        rec[f"{k}_ms"] = spread(times[k])
        rec[f"{k}_all_ms"] = [round(t, 4) for t in times[k]]
        rec[f"{k}_pairs_per_s"] = round(pairs / med, 1)
        rec[f"{k}_share_of_valu_ceiling"] = round(
            pairs * OPS_PER_PAIR / med / VALU_LANE_OPS, 4)
    rec["argsort2_ms"] = spread(times["argsort2"])
    rec["argsort2_all_ms"] = [round(t, 4) for t in times["argsort2"]]
    rec["ratio_to_argsort2"] = round(
        statistics.median(times["argsort2"])
        / statistics.median(times["rank"]), 3)
    rec["baseline_note"] = ("argsort2 gives ordinal ranks: it ignores ties, "
                            "so it does less work than rank_columns")
    return rec


def bench_phase(dev: torch.device) -> dict:
    """graphs_walks_overlapped at the ex shape, corr pearson vs spearman."""
    from g2vec_amd import io as gio
    from g2vec_amd import preprocess as pp
    from g2vec_amd.config import G2VecConfig
    from g2vec_amd.parallel.dist import single
    from g2vec_amd.pipeline import generate_paths
    from g2vec_amd.utils.obs import PhaseTimers
    from g2vec_amd.utils.synth import make_ex_style_files
    rec = {"shape": "ex_phase"}
    with tempfile.TemporaryDirectory() as tmp:
        files = make_ex_style_files(tmp)
        data = gio.load_expression(files["expression"])
        clinical = gio.load_clinical(files["clinical"])
        network = gio.load_network(files["network"])
        data["label"] = pp.match_labels(clinical, data["sample"])
        common = pp.find_common_genes(network["gene"], data["gene"])
        network = pp.restrict_network(network, common)
        data = pp.restrict_data(data, common)
        edge_idx = pp.edges_to_indices(network["edge"], common)
    n_samples, n_genes = data["expr"].shape
    rec.update(S=int(n_samples), G=int(n_genes), n_edges=int(len(edge_idx)))
    expr_t = torch.from_numpy(data["expr"]).to(dev)
    labels_t = torch.from_numpy(np.asarray(data["label"])).to(dev)
    edge_t = torch.from_numpy(edge_idx).to(dev)
    ctx = single(dev)
    kinds = ("pearson", "spearman")
    phase = {k: [] for k in kinds}
    wall = {k: [] for k in kinds}
    nnz = {}
    for i in range(PHASE_WARM + PHASE_REPS):    # interleaved run by run
        for corr in kinds:
            cfg = G2VecConfig(corr=corr, device="cuda", seed=0)
            timers = PhaseTimers()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, _, stats = generate_paths(cfg, expr_t, labels_t, edge_t,
                                            n_genes, ctx, timers=timers)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            nnz[corr] = (int(stats["nnz_g0"]), int(stats["nnz_g1"]))
            if i >= PHASE_WARM:
                wall[corr].append(dt * 1e3)
                phase[corr].append(
                    timers.summary()["graphs_walks_overlapped"] * 1e3)
    for corr in kinds:
        rec[corr] = {"graphs_walks_overlapped_ms": spread(phase[corr]),
                     "generate_paths_wall_ms": spread(wall[corr]),
                     "runs": PHASE_REPS, "warm_runs": PHASE_WARM,
                     "nnz_g0": nnz[corr][0], "nnz_g1": nnz[corr][1]}
    return rec


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="ex68,ex,200k,1m",
                    help="comma list of " + "/".join(SHAPES) + " (or none)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--phase", action="store_true",
                    help="also time steps 2b-3 at the ex shape per corr")
    ap.add_argument("--out-prefix", default="",
                    help="also write PREFIX<shape>.json per shape")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_rank needs a GPU: nothing measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    recs = []
    for name in [s for s in args.shapes.split(",") if s and s != "none"]:
        S, G = SHAPES[name]
        recs.append(bench_shape(name, S, G, args.reps, args.warm, dev))
        print(json.dumps(recs[-1]), flush=True)
    if args.phase:
        recs.append(bench_phase(dev))
        print(json.dumps(recs[-1]), flush=True)
    if args.out_prefix:
        for rec in recs:
            with open(f"{args.out_prefix}{rec['shape']}.json", "w") as fh:
                fh.write(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
