#!/usr/bin/env python3
"""A/B timing of steps 5-6: torch vs hip k-means and host vs device scoring
on synthetic blob embeddings, one process, warmed, interleaved repeats.

Per shape (G genes x h columns; default the ex shape 7.5k x 128 and the
scale shapes 200k x 256 and 1M x 512) it prints one JSON line with

  kmeans.torch / kmeans.hip   total seconds per repeat (median + all);
                              hip_1restart is n_init=1, the like-for-like
                              of kmeans_torch's single initialisation
  kmeans.hip_iterations       Lloyd steps summed over the restarts
  kmeans.hip_step_s           device-event time of ONE kmeans_step (median)
  kmeans.hip_step_bytes_per_s G*h*4 bytes (the one streamed read of X)
                              over that time, and its share of 6.3 TB/s
  kmeans.inertia_*            hip vs sklearn (G <= 50k) or torch (above)
  scoring.host / .device      seconds per repeat for the d- and t-score
                              vectors of all genes (NumPy vs the kernels
                              plus their two [G] copies to the host)

The yardstick is the project's own earlier path in the same process on the
same machine; nothing here asserts a speed. Needs a GPU: without one it
stops instead of timing the CPU mirrors."""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from g2vec_amd import cluster, ops, scoring  # noqa: E402

HBM_ACHIEVABLE = 6.3e12      # bytes/s, streaming (docs/KERNELS.md roofline)
SHAPES = {"ex": (7523, 128), "200k": (200_000, 256), "1m": (1_000_000, 512)}


def blob_embeddings(G: int, h: int, seed: int = 0) -> torch.Tensor:
    """Three overlapping blobs (10 / 20 / 70 % of the rows) with per-row
    scale jitter: enough overlap that Lloyd needs tens of steps."""
    gen = torch.Generator().manual_seed(seed)
    centres = torch.randn(3, h, generator=gen) * 0.6
    which = torch.bucketize(torch.rand(G, generator=gen),
                            torch.tensor([0.1, 0.3]))
    X = torch.randn(G, h, generator=gen)
    X *= 0.5 + torch.rand(G, 1, generator=gen)
    return (X + centres[which]).contiguous()


def inertia_of(X: torch.Tensor, labels) -> float:
    """f64 inertia of a labelling against its own cluster means."""
    lab = torch.as_tensor(labels, device=X.device).long()
    tot = 0.0
    for j in range(3):
        rows = X[lab == j].double()
        if rows.shape[0]:
            tot += float(((rows - rows.mean(dim=0)) ** 2).sum())
    return tot


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def timed(fn):
    _sync()
    t0 = time.perf_counter()
    out = fn()
    _sync()
    return time.perf_counter() - t0, out


def step_time(X: torch.Tensor, k: int = 3, reps: int = 20) -> float:
    """Median device-event seconds of one kmeans_step (both launches)."""
    G, h = X.shape
    C = X[:k].clone()
    labels = torch.zeros(G, dtype=torch.int32, device=X.device)
    sums = torch.empty(k, h, device=X.device)
    counts = torch.empty(k, dtype=torch.int32, device=X.device)
    chg = torch.empty(1, dtype=torch.int32, device=X.device)
    inert = torch.empty(1, dtype=torch.float64, device=X.device)
    times = []
    for i in range(reps + 3):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        ops.kmeans_step(X, C, labels, labels, C, sums, counts, chg, inert)
        b.record()
        b.synchronize()
        if i >= 3:
            times.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(times)


def bench_shape(name: str, G: int, h: int, S: int, repeats: int,
                n_init: int, dev: torch.device) -> dict:
    X_host = blob_embeddings(G, h)
    X = X_host.to(dev)
    W_np = X_host.numpy()
    rng = np.random.default_rng(1)
    expr = rng.normal(size=(S, G)).astype(np.float32)
    labels = (np.arange(S) % 5 < 2).astype(np.int64)
    expr_t = torch.from_numpy(expr).to(dev)
    labels_t = torch.from_numpy(labels).to(dev)

    def km_torch():
        # the torch backend as pipeline.run drives it: host array in,
        # copied to the device inside
        Xd = torch.from_numpy(W_np).to(dev)
        return cluster.kmeans_torch(Xd, 3, seed=0)

    def km_hip():
        return cluster.kmeans_hip(X, 3, seed=0, n_init=n_init)

    def sc_host():
        return (np.linalg.norm(W_np, axis=1), scoring.t_scores(expr, labels))

    def sc_dev():
        return (ops.row_norms(X).cpu().numpy(),
                ops.t_scores(expr_t, labels_t).cpu().numpy())

    def km_hip1():
        # one restart: the like-for-like of kmeans_torch's single init
        return cluster.kmeans_hip(X, 3, seed=0, n_init=1)

    runs = {"kmeans_torch": km_torch, "kmeans_hip": km_hip,
            "kmeans_hip1": km_hip1,
            "scoring_host": sc_host, "scoring_device": sc_dev}
    last = {}
    for fn in runs.values():                       # warm every path once
        timed(fn)
    times = {k: [] for k in runs}
    for _ in range(repeats):                       # interleaved A/B
        for key, fn in runs.items():
            dt, last[key] = timed(fn)
            times[key].append(dt)

    hip_labels, _c, hip_inertia, _n = last["kmeans_hip"]
    # steps summed over restarts, counted by a replay of the same seeds
    bufs = cluster._lloyd_buffers(X, 3, 300)
    n_steps = sum(cluster._lloyd(X, cluster._kpp_init(X, 3, 0, r), 300, 4,
                                 bufs)[3] for r in range(n_init))
    if G <= 50_000:
        from sklearn.cluster import KMeans
        km = KMeans(n_clusters=3, random_state=0, n_init=10).fit(W_np)
        other = ("sklearn", float(km.inertia_))
    else:
        other = ("torch", inertia_of(X, last["kmeans_torch"]))
    st = step_time(X)
    bps = G * h * 4 / st
    d_h, t_h = last["scoring_host"]
    d_d, t_d = last["scoring_device"]

    def med(key):
        return round(statistics.median(times[key]), 6)

    return {
        "shape": name, "G": G, "h": h, "S": S, "repeats": repeats,
        "device": (torch.cuda.get_device_name(0) if dev.type == "cuda"
                   else "cpu"),
        "kmeans": {
            "torch_s": med("kmeans_torch"),
            "torch_all_s": [round(x, 6) for x in times["kmeans_torch"]],
            "hip_s": med("kmeans_hip"),
            "hip_all_s": [round(x, 6) for x in times["kmeans_hip"]],
            "hip_1restart_s": med("kmeans_hip1"),
            "hip_1restart_all_s": [round(x, 6) for x in times["kmeans_hip1"]],
            "hip_1restart_iterations": last["kmeans_hip1"][3],
            "hip_n_init": n_init, "hip_iterations": n_steps,
            "hip_s_per_iteration_incl_init":
                round(statistics.median(times["kmeans_hip"]) / n_steps, 9),
            "hip_step_s": round(st, 9),
            "hip_step_bytes_per_s": round(bps, 0),
            "hip_step_share_of_6.3TBps": round(bps / HBM_ACHIEVABLE, 4),
            "inertia_hip": hip_inertia,
            "inertia_hip_f64_recomputed": inertia_of(X, hip_labels),
            "inertia_" + other[0]: other[1],
        },
        "scoring": {
            "host_s": med("scoring_host"),
            "host_all_s": [round(x, 6) for x in times["scoring_host"]],
            "device_s": med("scoring_device"),
            "device_all_s": [round(x, 6) for x in times["scoring_device"]],
            "max_abs_diff_d": float(np.abs(d_h - d_d).max()),
            "max_abs_diff_t": float(np.abs(t_h - t_d).max()),
        },
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="ex,200k,1m",
                    help="comma list of " + "/".join(SHAPES))
    ap.add_argument("--samples", type=int, default=135)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-init", type=int, default=10)
    ap.add_argument("--out-prefix", default="",
                    help="also write PREFIX<shape>.json per shape")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_steps56 needs a GPU: nothing measured", file=sys.stderr)
        return 2
    for name in args.shapes.split(","):
        G, h = SHAPES[name]
        rec = bench_shape(name, G, h, args.samples, args.repeats,
                          args.n_init, torch.device("cuda", 0))
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out_prefix:
            with open(f"{args.out_prefix}{name}.json", "w") as fh:
                fh.write(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
