#!/usr/bin/env python3
"""Time the device sums of the tally on a grid that does not fit the Infinity Cache.

    rocprofv3 --kernel-trace --stats -d DIR -o tally --output-format csv -- python tools/tally_sums_time.py
    python tools/tally_sums_time.py --summarise DIR/.../tally_kernel_trace.csv

The run sets a 512^3 u64 fixed-point grid (1 GiB: every pass over it comes from HBM), fills it with one short launch, and
calls the depth profile (mask 4), the projections along z (mask 3) and x (mask 6), the grid total (mask 0) and one r-z map
of 363 rings, each CALLS times after WARMUP warm-up calls, then read_grid() once -- whose k_grid_to_f64 streams the same
grid and writes as much again: the yardstick -- and the r-z map again after one unit has been added to every voxel (the map
skips empty voxels, which most of a traced grid are).  It prints the host's wall time per call (launches, the copy of the result
and the synchronisation included).  --summarise reads the kernel trace of such a run: every call ends with one
k_sum_finish, so the dispatches between two of them are one call's kernels; it prints, per sum, the summed duration of its
kernels per call and the bytes of grid per second that amounts to."""
import argparse
import csv
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, WARMUP, CALLS = 512, 2, 10
SUMS = ["mask 4 (depth profile)", "mask 3 (projection along z)", "mask 6 (projection along x)", "mask 0 (grid total)",
        "r-z map, 363 rings", "r-z map, no voxel empty"]
GRID_BYTES = N ** 3 * 8


def run(photons):
    import light_transport_amd as lt
    ctx = lt.Context(0)
    voxel = 25.6 / N
    ctx.set_media([(0.1, 10.0, 0.9, 1.0)])
    ctx.set_layers([0.0, np.inf], [0])
    ctx.set_grid((N, N, N), (-12.8, -12.8, 0.0), (voxel,) * 3, "u64fx")
    ctx.set_source(lt._lib.SRC_PENCIL, (0, 0, 0), (0, 0, 1))
    ctx.set_tally_mode("atomic")
    ctx.launch(photons, seed=0)
    ctx.sync()
    bins = lt.radial_bins((N, N), (-12.8, -12.8), (voxel, voxel), (0.0, 0.0), voxel, 362)       # 362 rings + the rest = 363 bins
    calls = [lambda: ctx.tally_sum(4), lambda: ctx.tally_sum(3), lambda: ctx.tally_sum(6), lambda: ctx.tally_sum(0),
             lambda: ctx.tally_sum_columns(bins, 363)]
    results = []

    def timed(name, f):
        for _ in range(WARMUP):
            f()
        t = []
        for _ in range(CALLS):
            t0 = time.perf_counter()
            r = f()
            t.append(time.perf_counter() - t0)
        results.append(r)
        print("%-30s host wall per call: median %.3f ms, min %.3f ms" % (name, 1e3 * float(np.median(t)), 1e3 * min(t)))
    for name, f in zip(SUMS, calls):
        timed(name, f)
    t0 = time.perf_counter()
    g = ctx.read_grid()
    print("%-30s host wall: %.1f ms (1 GiB converted on the device, 1 GiB copied to the host)" % ("read_grid()", 1e3 * (time.perf_counter() - t0)))
    # the sums agree with the grid they were taken from (u64 fixed point: exactly)
    total = float(results[3])
    assert total > 0 and np.allclose(results[0], g.sum(axis=(1, 2)), rtol=1e-12, atol=0.0)
    assert abs(results[0].sum() - total) <= 1e-12 * total and abs(results[4].sum() - total) <= 1e-12 * total
    print("grid total %.6f units of weight from %d photons; depth profile, r-z map and total agree with read_grid()" % (total, photons))
    # the traced grid is mostly empty, and the r-z map skips empty voxels: once more with one unit added to every voxel, so
    # that every voxel costs its LDS add
    raw = ctx.read_grid_raw()
    print("%.2f %% of the traced grid's voxels hold something" % (100.0 * np.count_nonzero(raw) / raw.size))
    raw += np.uint64(1)
    ctx.write_grid(raw)
    timed(SUMS[5], calls[4])
    assert np.allclose(results[5].sum(axis=1), results[4].sum(axis=1) + N * N * 2.0 ** -40, rtol=1e-12, atol=0.0)
    ctx.close()


def summarise(path):
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    calls, cur, yard = [], [], []
    for t0, t1, name in rows:
        if "k_grid_to_f64" in name:
            yard.append(t1 - t0)
        if "k_sum_" not in name:
            continue
        cur.append((re.search(r"k_sum_[a-z]+", name).group(0), t1 - t0))
        if "k_sum_finish" in name:
            calls.append(cur)
            cur = []
    per = WARMUP + CALLS
    if len(calls) != per * len(SUMS) or len(yard) != 1:
        raise SystemExit("expected %d calls and one k_grid_to_f64 in the trace, found %d and %d" % (per * len(SUMS), len(calls), len(yard)))
    print("k_grid_to_f64 (yardstick): %.1f us, reads %d and writes %d bytes: %.2f TB/s" % (yard[0] / 1e3, GRID_BYTES, GRID_BYTES, 2 * GRID_BYTES / yard[0] / 1e3))
    for i, name in enumerate(SUMS):
        mine = calls[i * per + WARMUP:(i + 1) * per]
        tot = [sum(d for _, d in c) for c in mine]
        kern = ", ".join("%s %.1f us" % (k, float(np.mean([c[j][1] for c in mine])) / 1e3) for j, (k, _) in enumerate(mine[0]))
        print("%-30s kernels per call: mean %.1f us, min %.1f us, max %.1f us = %.2f TB/s of grid   [%s]" % (
            name, float(np.mean(tot)) / 1e3, min(tot) / 1e3, max(tot) / 1e3, GRID_BYTES / float(np.mean(tot)) / 1e3, kern))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="summarise the kernel trace of a profiled run instead of running")
    ap.add_argument("--photons", type=int, default=1 << 20, help="photons of the launch that fills the grid")
    a = ap.parse_args()
    summarise(a.summarise) if a.summarise else run(a.photons)
