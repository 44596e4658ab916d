#!/usr/bin/env python3
"""Time the batch statistics of the tally (fold and class summary) on a grid that does not fit the Infinity Cache.

    rocprofv3 --kernel-trace --stats -d DIR -o stats --output-format csv -- python tools/tally_stats_time.py
    python tools/tally_stats_time.py --summarise DIR/.../stats_kernel_trace.csv

The run sets a 512^3 u64 fixed-point grid (1 GiB: every pass over it comes from HBM) with statistics on (prev: 1 GiB, m2:
1 GiB) and does, in this order:
  1. WARMUP + CALLS batches of photons, a fold after each           -- "fold, traced batch": almost every 16-byte group unchanged
  2. the class summary WARMUP + CALLS times                         -- "summary, traced grid": empty groups do not read m2
  3. WARMUP + CALLS times: one unit added to every voxel on the host, the grid written back, a fold
                                                                    -- "fold, every voxel changed": 40 bytes per voxel
  4. the class summary WARMUP + CALLS times                         -- "summary, no voxel empty": 16 bytes per voxel
  5. the depth profile (lt_tally_sum_axes, mask 4) WARMUP + CALLS times -- the yardstick: one read of the grid
It checks the results against NumPy on the way and prints host wall times.  --summarise reads the kernel trace of such a run
and prints, per item, the kernel time per call and the bytes per second that amounts to under the traffic model named."""
import argparse
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, WARMUP, CALLS = 512, 1, 5
EDGES = [0.05, 0.1, 0.2, 0.5]
VOXELS = N ** 3
GRID_BYTES = VOXELS * 8


def run(photons):
    import light_transport_amd as lt
    ctx = lt.Context(0)
    voxel = 25.6 / N
    ctx.set_media([(0.1, 10.0, 0.9, 1.0)])
    ctx.set_layers([0.0, np.inf], [0])
    ctx.set_grid((N, N, N), (-12.8, -12.8, 0.0), (voxel,) * 3, "u64fx")
    ctx.set_source(lt._lib.SRC_PENCIL, (0, 0, 0), (0, 0, 1))
    ctx.set_tally_mode("atomic")
    ctx.stats_enable()
    per = WARMUP + CALLS

    def wall(name, f, prepare=None):
        t = []
        for _ in range(per):
            if prepare:
                prepare()
            ctx.sync()
            t0 = time.perf_counter()
            r = f()
            ctx.sync()
            t.append(time.perf_counter() - t0)
        print("%-28s host wall per call: median %.3f ms, min %.3f ms" % (name, 1e3 * float(np.median(t[WARMUP:])), 1e3 * min(t[WARMUP:])))
        return r
    batch = [0]

    def trace_a_batch():
        ctx.launch(photons, seed=0, photon_offset=photons * batch[0])
        batch[0] += 1
    wall("fold, traced batch", ctx.stats_fold, trace_a_batch)
    vox, raw_w = wall("summary, traced grid", lambda: ctx.stats_summary(EDGES, raw=True))
    raw = ctx.read_grid_raw()
    filled = int(np.count_nonzero(raw))
    assert int(vox.sum()) == VOXELS and int(vox[-1]) == VOXELS - filled and int(raw_w.sum()) == int(raw.sum(dtype=np.uint64))
    print("%d batches of %d photons: %.2f %% of the voxels hold something; voxels per class %s" % (
        per, photons, 100.0 * filled / VOXELS, vox.tolist()))
    share = raw_w[:-1].astype(np.float64).cumsum() / float(raw_w.sum())
    print("share of the absorbed weight below %s relative error: %s" % (EDGES, ["%.4f" % s for s in share[:len(EDGES)]]))

    def one_more_everywhere():
        raw[...] += np.uint64(1)
        ctx.write_grid(raw)
    wall("fold, every voxel changed", ctx.stats_fold, one_more_everywhere)
    vox2, raw_w2 = wall("summary, no voxel empty", lambda: ctx.stats_summary(EDGES, raw=True))
    assert int(vox2.sum()) == VOXELS and vox2[-1] == 0 and int(raw_w2.sum()) == int(raw.sum(dtype=np.uint64))
    assert ctx.stats_batches() == 2 * per
    prof = wall("depth profile (yardstick)", lambda: ctx.tally_sum(4, raw=True))
    assert int(prof.sum(dtype=np.uint64)) == int(raw.sum(dtype=np.uint64))
    ctx.close()


def summarise(path):
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    folds = [t1 - t0 for t0, t1, n in rows if "k_stats_fold" in n]
    classes = [t1 - t0 for t0, t1, n in rows if "k_stats_classes" in n]
    yard = [(t1 - t0) + (rows[i + 1][1] - rows[i + 1][0]) for i, (t0, t1, n) in enumerate(rows) if "k_sum_rows" in n]      # + its k_sum_finish
    per = WARMUP + CALLS
    if len(folds) != 2 * per or len(classes) != 2 * per or len(yard) != per:
        raise SystemExit("expected %d folds, %d summaries and %d depth profiles in the trace, found %d, %d and %d" % (
            2 * per, 2 * per, per, len(folds), len(classes), len(yard)))
    items = [("fold, traced batch", folds[WARMUP:per], 2 * GRID_BYTES, "grid + prev read: 16 B/voxel"),
             ("fold, every voxel changed", folds[per + WARMUP:], 5 * GRID_BYTES, "grid, prev, m2 read, prev, m2 written: 40 B/voxel"),
             ("summary, traced grid", classes[WARMUP:per], GRID_BYTES, "prev read: 8 B/voxel (m2 only where something is)"),
             ("summary, no voxel empty", classes[per + WARMUP:], 2 * GRID_BYTES, "prev + m2 read: 16 B/voxel"),
             ("depth profile (yardstick)", yard[WARMUP:], GRID_BYTES, "grid read: 8 B/voxel")]
    for name, t, nbytes, model in items:
        print("%-28s kernel time per call: mean %.1f us, min %.1f us, max %.1f us = %.2f TB/s   [%s]" % (
            name, float(np.mean(t)) / 1e3, min(t) / 1e3, max(t) / 1e3, nbytes / float(np.mean(t)) / 1e3, model))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="summarise the kernel trace of a profiled run instead of running")
    ap.add_argument("--photons", type=int, default=1 << 18, help="photons per batch")
    a = ap.parse_args()
    summarise(a.summarise) if a.summarise else run(a.photons)
