#!/usr/bin/env python3
"""Time the box read-out of the tally (lt_tally_box) on the 256^3 grid of C2 and on a 512^3 grid.

    rocprofv3 --kernel-trace --stats -d DIR -o box --output-format csv -- python tools/time_tally_box.py
    python tools/time_tally_box.py --summarise DIR/.../box_kernel_trace.csv

For every grid size and for an f64 and a u64 fixed-point tally the run sets C2's slab, fills the grid with one short launch, and
calls, each CALLS times after WARMUP warm-up calls: the whole grid at bins 2^3, 4^3 and 16^3, the central y-slice, a 64^3 box in
the middle at bin 1, and the depth profile (lt_tally_sum_axes, keep = z), which streams the same grid once: the bandwidth
yardstick.  It prints the host's wall time per call (the copy of the result included) and the bytes of the result against the
grid's.  --summarise reads the kernel trace of such a run and prints, per call, the kernel time and the bytes of the grid read
per second."""
import argparse
import csv
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES, DTYPES, WARMUP, CALLS = [256, 512], ["f64", "u64fx"], 1, 5


def plan(n):
    """(label, lo, size, bin) of the box calls on an n^3 grid; the yardstick follows them."""
    whole, mid = (n, n, n), n // 2 - 32
    return [("whole grid, bin 2^3", (0, 0, 0), whole, (2, 2, 2)), ("whole grid, bin 4^3", (0, 0, 0), whole, (4, 4, 4)),
            ("whole grid, bin 16^3", (0, 0, 0), whole, (16, 16, 16)), ("central y-slice", (0, n // 2, 0), (n, 1, n), (1, 1, 1)),
            ("64^3 box, bin 1", (mid, mid, mid), (64, 64, 64), (1, 1, 1))]


YARDSTICK = "depth profile (lt_tally_sum_axes)"


def run(photons):
    import light_transport_amd as lt
    from light_transport_amd import _lib
    ctx = lt.Context(0)

    def timed(name, f):
        for _ in range(WARMUP):
            f()
        t = []
        for _ in range(CALLS):
            t0 = time.perf_counter()
            r = f()
            t.append(time.perf_counter() - t0)
        print("%-36s host wall per call: median %8.2f ms, min %8.2f ms" % (name, 1e3 * float(np.median(t)), 1e3 * min(t)), flush=True)
        return r
    for n in SIZES:
        voxel = 25.6 / n
        for dtype in DTYPES:
            ctx.set_media([(0.1, 10.0, 0.9, 1.0)])
            ctx.set_layers([0.0, np.inf], [0])
            ctx.set_grid((n, n, n), (-12.8, -12.8, 0.0), (voxel,) * 3, dtype)
            ctx.set_source(_lib.SRC_PENCIL, (0.5 * voxel, 0.5 * voxel, 0), (0, 0, 1))
            ctx.launch(photons, seed=0)
            ctx.sync()
            grid_bytes = n ** 3 * 8
            print("-- %d^3 %s tally (%d MiB), %d photons" % (n, dtype, grid_bytes >> 20, photons), flush=True)
            total = None
            for name, lo, size, bin in plan(n):
                r = timed(name, lambda: ctx.tally_box(lo, size, bin))
                print("%-36s result %d bytes = 1 / %.0f of the grid" % ("", r.nbytes, grid_bytes / r.nbytes))
                if size == (n, n, n):
                    total = r.sum() if total is None else total
                    assert abs(r.sum() - total) <= 1e-9 * total          # every binning of the whole grid holds the grid's weight
            prof = timed(YARDSTICK, lambda: ctx.tally_sum(4))
            assert abs(prof.sum() - total) <= 1e-9 * total
    ctx.close()


def summarise(path):
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    box = [(n, t1 - t0) for t0, t1, n in rows if "k_box_" in n]
    sums = [(n, t1 - t0) for t0, t1, n in rows if "k_sum_" in n]
    per = WARMUP + CALLS

    def take(src, k, name, read_bytes):
        if len(src) < per * k:
            raise SystemExit("the trace holds fewer kernels than the plan of run(): %s" % name)
        mine, src[:] = src[:per * k], src[per * k:]
        calls = [mine[i * k:(i + 1) * k] for i in range(WARMUP, per)]
        tot = [sum(d for _, d in c) for c in calls]
        kern = ", ".join(re.search(r"k_[a-z_]+(<[^>]*>)?", c).group(0) for c, _ in calls[0])
        print("%-36s kernels per call: mean %8.1f us, min %8.1f us, max %8.1f us; reads %10d bytes: %.2f TB/s at the mean   [%s]" % (
            name, float(np.mean(tot)) / 1e3, min(tot) / 1e3, max(tot) / 1e3, read_bytes, read_bytes / float(np.mean(tot)) / 1e3, kern))
    for n in SIZES:
        for dtype in DTYPES:
            print("-- %d^3 %s tally" % (n, dtype))
            for name, _, size, _ in plan(n):
                take(box, 1, name, size[0] * size[1] * size[2] * 8)
            take(sums, 2, YARDSTICK, n ** 3 * 8)
    if box or sums:
        print("NOTE: the trace holds %d + %d more kernels than the plan of run(): the rows above may be shifted" % (len(box), len(sums)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="summarise the kernel trace of a profiled run instead of running")
    ap.add_argument("--photons", type=int, default=1 << 20, help="photons of the launch that fills the grid")
    a = ap.parse_args()
    summarise(a.summarise) if a.summarise else run(a.photons)
