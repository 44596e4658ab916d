#!/usr/bin/env python3
"""Time the convolution of the tally (lt_tally_convolve*) on the 256^3 grid of C2.

    rocprofv3 --kernel-trace --stats -d DIR -o conv --output-format csv -- python tools/tally_conv_time.py
    python tools/tally_conv_time.py --summarise DIR/.../conv_kernel_trace.csv

The run sets C2's slab and grid (256^3 voxels of 0.1, the pencil in the centre of column (128, 128)) with an f64 and then a
u64 fixed-point tally, fills it with one short launch, and calls, each CALLS times after WARMUP warm-up calls: the separable
form with the 33 + 33 taps of a Gaussian beam, the 2-D form with the 33 x 33 taps of a flat-top beam and with 63 x 63 taps, the
_at form with 63 x 63 taps at 8 columns, and the depth profile (lt_tally_sum_axes, mask 4), which streams the same grid once: the
bandwidth yardstick.  Then read_grid() once (k_grid_to_f64 where the tally is not f64, and the copy to the host): the only route
to a finite-beam result without these calls.  With the u64 tally the two 2-D calls run once more after one unit has been added
to every voxel, so that no tile is skipped.  It prints the host's wall time per call (the copy of the result included: 128 MiB
for the whole grid).  --summarise reads the kernel trace of such a run and prints the kernel time per call."""
import argparse
import csv
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, WARMUP, CALLS = 256, 1, 5
# (label, kernels of lt_tallyconv.hip per call, kernels of lt_tallysum.hip per call)
PLAN = [("separable, Gaussian 33 + 33", 2, 0), ("2-D, flat-top 33 x 33", 1, 0), ("2-D, 63 x 63", 1, 0), ("_at, 63 x 63 at 8 columns", 1, 0),
        ("depth profile (lt_tally_sum_axes)", 0, 2)]
FULL = [("2-D, flat-top 33 x 33, no tile skipped", 1, 0), ("2-D, 63 x 63, no tile skipped", 1, 0)]
DTYPES = ["f64", "u64fx"]


def run(photons):
    import light_transport_amd as lt
    from light_transport_amd.src.beam_profiles import FlatTopProfile, GaussianProfile
    ctx = lt.Context(0)
    voxel = 25.6 / N
    gauss = GaussianProfile(0.64).taps((voxel, voxel))             # 2.5 radii = 16 columns either side
    flat = FlatTopProfile(1.6).taps((voxel, voxel))
    big = np.random.RandomState(0).random_sample((63, 63))
    assert gauss[0].size == gauss[1].size == 33 and flat.shape == (33, 33)
    cols = np.array([[128, 128], [129, 128], [132, 128], [140, 128], [160, 128], [200, 128], [128, 0], [255, 255]], dtype=np.int32)
    calls = [lambda: ctx.tally_convolve(gauss), lambda: ctx.tally_convolve(flat), lambda: ctx.tally_convolve(big),
             lambda: ctx.tally_convolve_at(big, cols), lambda: ctx.tally_sum(4)]

    def timed(name, f):
        for _ in range(WARMUP):
            f()
        t = []
        for _ in range(CALLS):
            t0 = time.perf_counter()
            r = f()
            t.append(time.perf_counter() - t0)
        print("%-42s host wall per call: median %.2f ms, min %.2f ms" % (name, 1e3 * float(np.median(t)), 1e3 * min(t)))
        return r
    for dtype in DTYPES:
        ctx.set_media([(0.1, 10.0, 0.9, 1.0)])
        ctx.set_layers([0.0, np.inf], [0])
        ctx.set_grid((N, N, N), (-12.8, -12.8, 0.0), (voxel,) * 3, dtype)
        ctx.set_source(lt._lib.SRC_PENCIL, (0.5 * voxel, 0.5 * voxel, 0), (0, 0, 1))
        ctx.launch(photons, seed=0)
        ctx.sync()
        print("-- %s tally, %d photons" % (dtype, photons))
        res = [timed(name, f) for (name, _, _), f in zip(PLAN, calls)]
        t0 = time.perf_counter()
        g = ctx.read_grid()
        print("%-42s host wall: %.1f ms" % ("read_grid()", 1e3 * (time.perf_counter() - t0)))
        nonzero = g != 0
        tiles = nonzero.reshape(N, N // 32, 32, N // 32, 32).any(axis=(2, 4))
        print("%.2f %% of the voxels and %.1f %% of the 32 x 32 tiles hold something" % (100.0 * nonzero.mean(), 100.0 * tiles.mean()))
        # the calls agree with one another and with the grid they were taken from
        total = g.sum()
        assert abs(res[4].sum() - total) <= 1e-9 * total
        assert 0.9 * total < res[0].sum() <= total * gauss[0].sum() * gauss[1].sum() * (1 + 1e-9) and res[1].sum() <= total * (1 + 1e-9)      # the edges only lose
        assert np.allclose(res[3], res[2][:, cols[:, 1], cols[:, 0]], rtol=1e-11, atol=0.0)
        if dtype == "u64fx":
            raw = ctx.read_grid_raw()
            raw += np.uint64(1)
            ctx.write_grid(raw)
            for (name, _, _), f in zip(FULL, calls[1:3]):
                timed(name, f)
    ctx.close()


def summarise(path):
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    conv = [(n, t1 - t0) for t0, t1, n in rows if "k_conv_" in n]
    sums = [(n, t1 - t0) for t0, t1, n in rows if "k_sum_" in n]
    for n, d in ((n, t1 - t0) for t0, t1, n in rows if "k_grid_to_f64" in n):
        print("k_grid_to_f64 (read_grid() of the u64 tally, before its copy): %.1f us, reads and writes %d bytes: %.2f TB/s" % (
            d / 1e3, N ** 3 * 8, 2 * N ** 3 * 8 / d / 1e3))
    per = WARMUP + CALLS
    for dtype in DTYPES:
        print("-- %s tally" % dtype)
        for name, n_conv, n_sum in PLAN + (FULL if dtype == "u64fx" else []):
            src, k = (conv, n_conv) if n_conv else (sums, n_sum)
            if len(src) < per * k:
                raise SystemExit("the trace holds fewer kernels than the plan of run(): %s" % name)
            mine, src[:] = src[:per * k], src[per * k:]
            calls = [mine[i * k:(i + 1) * k] for i in range(WARMUP, per)]
            tot = [sum(d for _, d in c) for c in calls]
            kern = ", ".join("%s %.1f us" % (re.search(r"k_[a-z_]+(<[^>]*>)?", c).group(0), float(np.mean([cc[j][1] for cc in calls])) / 1e3)
                             for j, (c, _) in enumerate(calls[0]))
            print("%-42s kernels per call: mean %.1f us, min %.1f us, max %.1f us   [%s]" % (
                name, float(np.mean(tot)) / 1e3, min(tot) / 1e3, max(tot) / 1e3, kern))
    if conv or sums:
        print("NOTE: the trace holds %d + %d more kernels than the plan of run(): the rows above may be shifted" % (len(conv), len(sums)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="summarise the kernel trace of a profiled run instead of running")
    ap.add_argument("--photons", type=int, default=1 << 20, help="photons of the launch that fills the grid")
    a = ap.parse_args()
    summarise(a.summarise) if a.summarise else run(a.photons)
