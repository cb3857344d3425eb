#!/usr/bin/env python3
"""ms / epoch of the replica-batched epoch body (ReplicaTrainer.run_epoch)
next to R x the single trainer's epoch (CbowTrainer.run_epoch), on synthetic
path sets (utils/synth.synth_pathset), one process, warmed, interleaved.

Both sides run in the same regime: one accuracy readback per epoch and the
default graph setting (the body is replayed from a hipGraph from the second
epoch on). The yardstick is the SINGLE trainer as it stands: a batched run
at R is compared with R sequential single epochs, never with the batched
code at R = 1.

Per shape it prints one JSON line and, with --out-prefix, writes
PREFIX<shape>.json:

  rows[i].R                   replicas
  rows[i].batched_ms          median over --reps blocks of --epochs epochs of
                              (host clock around the block) / epochs; every
                              epoch ends in its device-to-host readback
  rows[i].single_ms           the same for one CbowTrainer, measured in the
                              same repeat loop, block by block alternating
  rows[i].R_x_single_ms       R * single_ms: R sequential single runs
  rows[i].batched_over_R_single   batched_ms / R_x_single_ms (< 1: the
                              batched epoch is cheaper than R single ones)
  rows[i].stream_gbps         R*G*h*4*6 bytes (W, m, v read and written) /
                              batched_ms: the Adam stream alone, against the
                              6.3 TB/s streaming ceiling

Nothing here asserts a speed. Needs a GPU: without one it stops instead of
timing the CPU mirrors."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from g2vec_amd.config import G2VecConfig  # noqa: E402
from g2vec_amd.models.cbow import CbowTrainer  # noqa: E402
from g2vec_amd.models.replicas import ReplicaTrainer  # noqa: E402
from g2vec_amd.paths import PathSet  # noqa: E402
from g2vec_amd.utils.synth import synth_pathset  # noqa: E402

# name -> (genes, paths, hidden, modules, replicas, epochs per block)
SHAPES = {"ex": (7523, 60_000, 128, 16, (1, 2, 4, 8, 16, 32), 200),
          "200k": (200_000, 2_000_000, 256, 64, (1, 4, 8), 20)}
QUIET = lambda *a, **k: None   # noqa: E731


def block_ms(step, n: int) -> float:
    """Host clock around n epochs; run_epoch ends in a readback, so the
    clock stops after the last epoch's device work."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def bench_shape(name: str, Rs, reps: int, warm: int, dev) -> dict:
    G, P, h, n_mod, default_Rs, n_ep = SHAPES[name]
    genes, offs, labels = synth_pathset(G, P, n_modules=n_mod, seed=1)
    ps = PathSet(torch.from_numpy(genes).to(dev),
                 torch.from_numpy(offs).to(dev),
                 torch.from_numpy(labels).to(dev), G)
    cfg = G2VecConfig(hidden=h, epochs=10 ** 6, seed=0, device="cuda")
    rows = []
    for R in (Rs or default_Rs):
        single = CbowTrainer(cfg, G, dev, log=QUIET)
        s_st = single.setup(ps)
        rep = ReplicaTrainer(cfg, G, dev, log=QUIET)
        r_st = rep.setup(ps, R)
        for _ in range(warm):                        # incl. graph capture
            single.run_epoch(s_st)
            rep.run_epoch(r_st)
        t_single, t_rep = [], []
        for _ in range(reps):                        # interleaved
            t_single.append(block_ms(lambda: single.run_epoch(s_st), n_ep))
            t_rep.append(block_ms(lambda: rep.run_epoch(r_st), n_ep))
        ms_s, ms_r = statistics.median(t_single), statistics.median(t_rep)
        rows.append({
            "R": R, "batched_ms": round(ms_r, 5), "single_ms": round(ms_s, 5),
            "R_x_single_ms": round(R * ms_s, 5),
            "batched_over_R_single": round(ms_r / (R * ms_s), 4),
            "stream_gbps": round(R * G * h * 24.0 / (ms_r * 1e-3) / 1e9, 1),
            "graph": [s_st.graph is not None, r_st.graph is not None],
            "batched_all_ms": [round(t, 5) for t in t_rep],
            "single_all_ms": [round(t, 5) for t in t_single]})
        print(f"[{name}] R={R}: batched {ms_r:.4f} ms/epoch, "
              f"{R} x single {R * ms_s:.4f}", file=sys.stderr, flush=True)
        del single, s_st, rep, r_st
        torch.cuda.empty_cache()
    return {"shape": name, "G": G, "P": P, "nnz": int(offs[-1]), "h": h,
            "epochs_per_block": n_ep, "reps": reps, "warm_epochs": warm,
            "regime": "per-epoch readback, hipGraph replay of the body",
            "device": torch.cuda.get_device_name(0), "rows": rows}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="ex,200k",
                    help="comma list of " + "/".join(SHAPES))
    ap.add_argument("--replicas", default="",
                    help="comma list of R (default: the shape's own list)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--out-prefix", default="",
                    help="also write PREFIX<shape>.json per shape")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_replicates needs a GPU: nothing measured",
              file=sys.stderr)
        return 2
    Rs = [int(x) for x in args.replicas.split(",") if x]
    for name in args.shapes.split(","):
        rec = bench_shape(name, Rs, args.reps, args.warm,
                          torch.device("cuda", 0))
        print(json.dumps(rec), flush=True)
        if args.out_prefix:
            with open(f"{args.out_prefix}{name}.json", "w") as fh:
                fh.write(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
