#!/usr/bin/env python3
"""Time the tally along rays (lt_tally_rays, lt_tally_view) on the 256^3 grid of C2 and on a 512^3 grid.

    rocprofv3 --kernel-trace --stats -d DIR -o rays --output-format csv -- python tools/tally_rays_time.py
    python tools/tally_rays_time.py --summarise DIR/.../rays_kernel_trace.csv

For every grid size and for a u64 fixed-point and an f64 tally the run sets C2's slab, fills the grid with one launch, and calls,
each CALLS times after WARMUP warm-up calls:
    (a) the line integral along z through every column centre (lt_tally_rays on n x n host-built rays): the numbers of
        lt_tally_sum_axes with keep = x, y -- checked against it -- by a walk instead of a streaming pass;
    (b) a 512 x 512 pinhole view (lt_tally_view) from outside the grid, looking along z: the integral alone, then all outputs;
    (c) the same camera distance, looking along (1, 1, 1): 45 degrees to all axes;
and the yardstick, lt_tally_sum_axes keep = x, y, which streams the same grid once, and read_grid().  It prints the host's wall
time per call (staging of the rays and the copy of the result included) and the voxels the rays of each view visit (worked out on
the host from the entry and exit voxel of every ray).  --summarise reads the kernel trace of such a run and prints, per call, the
kernel time, the voxel visits per second and (a)'s time over the yardstick's."""
import argparse
import csv
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES, DTYPES, WARMUP, CALLS, PIXELS = [256, 512], ["u64fx", "f64"], 1, 5, 512
EXTENT = 25.6
YARDSTICK = "yardstick: lt_tally_sum_axes keep = x, y"


def geometry(n):
    return (-0.5 * EXTENT, -0.5 * EXTENT, 0.0), (EXTENT / n,) * 3


def column_rays(n):
    origin, voxel = geometry(n)
    c = origin[0] + (np.arange(n) + 0.5) * voxel[0]
    o = np.empty((n, n, 3))
    o[..., 0], o[..., 1], o[..., 2] = c[None, :], c[:, None], -1.0
    return o.reshape(-1, 3), np.broadcast_to(np.array([0.0, 0.0, 1.0]), (n * n, 3)).copy()


def cameras():
    """(label, camera, f_distance, xs, ys): both 40 from the grid's centre, the field of view a little wider than the grid."""
    centre = np.array([0.0, 0.0, 0.5 * EXTENT])
    half = np.linspace(-0.45, 0.45, PIXELS)
    cam_z = centre - np.array([0.0, 0.0, 40.0])
    cam_d = centre - 40.0 / np.sqrt(3.0) * np.ones(3)
    return [("(b) pinhole view along z", cam_z, cam_z[2] + 1.0, cam_z[0] + half, cam_z[1] - half),
            ("(c) pinhole view along (1, 1, 1)", cam_d, cam_d[2] + 1.0, cam_d[0] + 1.0 + half, cam_d[1] + 1.0 - half)]


def voxel_visits(n, o, d):
    """The voxels the rays o + t d, t >= 0, visit in an n^3 grid: per ray 1 + the index steps between its entry and its exit."""
    origin, voxel = (np.asarray(v) for v in geometry(n))
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = (origin - o) / d, (origin + n * voxel - o) / d
    t0 = np.maximum(np.nanmax(np.minimum(a, b), axis=1), 0.0)
    t1 = np.nanmin(np.maximum(a, b), axis=1)
    hit = t1 > t0
    cell = lambda t: np.clip(np.floor((o + t[:, None] * d - origin) / voxel), 0, n - 1)      # noqa: E731
    return int(np.sum((1 + np.abs(cell(t1) - cell(t0)).sum(axis=1))[hit]))


def plan(n):
    """(label, voxel visits, kernel name) of the ray calls on an n^3 grid, in the order run() makes them."""
    from light_transport_amd import _lib
    rows = [("(a) columns along z, %d^2 rays" % n, n ** 3, "k_tally_rays")]
    for label, cam, f, xs, ys in cameras():
        o, d = _lib.camera_rays(cam, f, xs, ys)
        visits = voxel_visits(n, o.reshape(-1, 3), d.reshape(-1, 3))
        rows.append((label + ", integral", visits, "k_tally_view"))
        rows.append((label + ", all outputs", visits, "k_tally_view"))
    return rows


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
        print("%-52s host wall per call: median %8.2f ms, min %8.2f ms" % (name, 1e3 * float(np.median(t)), 1e3 * min(t)), flush=True)
        return r
    for n in SIZES:
        origin, voxel = geometry(n)
        o, d = column_rays(n)
        rows = plan(n)
        for dtype in DTYPES:
            ctx.set_media([(0.1, 10.0, 0.9, 1.0)])
            ctx.set_layers([0.0, np.inf], [0])
            ctx.set_grid((n, n, n), origin, voxel, dtype)
            ctx.set_source(_lib.SRC_PENCIL, (0.5 * voxel[0], 0.5 * voxel[0], 0), (0, 0, 1))
            ctx.launch(photons, seed=0)
            ctx.sync()
            print("-- %d^3 %s tally (%d MiB), %d photons" % (n, dtype, n ** 3 * 8 >> 20, photons), flush=True)
            col = timed(rows[0][0], lambda: ctx.tally_rays(o, d, want="integral")["integral"])
            k = 1
            for label, cam, f, xs, ys in cameras():
                for want in ("integral", _lib.RAY_WANTS):
                    r = timed(rows[k][0], lambda: ctx.tally_view(cam, f, xs, ys, threshold=1e-3, want=want))
                    print("%-52s %d voxel visits, %d of %d pixels see the grid" % ("", rows[k][1], np.count_nonzero(r["integral"]), PIXELS ** 2))
                    k += 1
            proj = timed(YARDSTICK, lambda: ctx.tally_sum(3))
            ref = proj.ravel() * voxel[2]
            assert np.all(np.abs(col - ref) <= (4 * n + 3) * 2.0 ** -52 * ref)          # (a) computes the yardstick's numbers
            timed("read_grid()", ctx.read_grid)
    ctx.close()


def summarise(path):
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    rays = [(n, t1 - t0) for t0, t1, n in rows if "k_tally_rays" in n or "k_tally_view" in n]
    sums = [(n, t1 - t0) for t0, t1, n in rows if "k_sum_" in n]
    per = WARMUP + CALLS

    def take(src, k, name):
        if len(src) < per * k:
            raise SystemExit("the trace holds fewer kernels than the plan of run(): %s" % name)
        mine, src[:] = src[:per * k], src[per * k:]
        calls = [mine[i * k:(i + 1) * k] for i in range(WARMUP, per)]
        tot = [sum(d for _, d in c) for c in calls]
        kern = ", ".join(re.search(r"k_[a-z_]+(<[^>]*>)?", c).group(0) for c, _ in calls[0])
        return float(np.mean(tot)), min(tot), max(tot), kern
    for n in SIZES:
        for dtype in DTYPES:
            print("-- %d^3 %s tally" % (n, dtype))
            first = None
            for name, visits, _ in plan(n):
                mean, lo, hi, kern = take(rays, 1, name)
                first = mean if first is None else first
                print("%-52s kernel: mean %9.1f us, min %9.1f us, max %9.1f us; %11d voxel visits: %7.2f G visits/s   [%s]" % (
                    name, mean / 1e3, lo / 1e3, hi / 1e3, visits, visits / mean, kern))
            mean, lo, hi, kern = take(sums, 2, YARDSTICK)
            print("%-52s kernels: mean %8.1f us, min %9.1f us, max %9.1f us; reads %d bytes: %.2f TB/s   [%s]" % (
                YARDSTICK, mean / 1e3, lo / 1e3, hi / 1e3, n ** 3 * 8, n ** 3 * 8 / mean / 1e3, kern))
            print("%-52s (a) over the yardstick: %.1f x" % ("", first / mean))
    if rays or sums:
        print("NOTE: the trace holds %d + %d more kernels than the plan of run(): the rows above may be shifted" % (len(rays), len(sums)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="summarise the kernel trace of a profiled run instead of running")
    ap.add_argument("--photons", type=int, default=1 << 20, help="photons of the launch that fills the grid")
    a = ap.parse_args()
    summarise(a.summarise) if a.summarise else run(a.photons)
