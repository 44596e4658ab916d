#!/usr/bin/env python3
"""How much did every structure absorb, where is its hottest voxel, and what share of its volume got at least dose D?  The
Cornell cavity with its cone (examples/cornell_cone.py, part 2) traced in batches and read out BY REGION on the device: the
label volume comes from the mesh itself (one ray per voxel centre), the totals, peaks and dose-volume histograms from one pass
over the tally each.  No grid is read back.

    python examples/region_dose.py [n_photons] [n_batches]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from light_transport_amd.src import constants as K
from light_transport_amd.src.bvh_new import build_linear_bvh
from light_transport_amd.src.cornell_box import get_cone, get_cornell_box, get_front_wall, get_light_quad
from light_transport_amd.src.photon_tracing import AreaLight, MeshVolume, OpticalMedium, PhotonTracer, VoxelGrid, set_triangle_media

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2 * 10 ** 6
batches = int(sys.argv[2]) if len(sys.argv) > 2 else 8
n -= n % batches
depth = 7.5
walls = set_triangle_media(get_cornell_box(depth, K.GLASS_MAT, K.GLASS_MAT, K.GLASS_MAT) + get_front_wall(depth, K.GLASS_MAT)
                           + get_light_quad(depth, K.GLASS_MAT), front=0, back=-1)     # normals point into the cavity
cone = set_triangle_media(get_cone(K.GLASS_MAT), front=0, back=1)                       # normals point out of the cone
primitives, linear_bvh = build_linear_bvh(walls + cone, 1)
volume = MeshVolume([OpticalMedium(0.1, 10.0, 0.9, 1.0), OpticalMedium(1.0, 5.0, 0.8, K.GLASS_MAT.ior)], start_medium=0)
grid = VoxelGrid((128, 128, 128), origin=(-depth,) * 3, voxel=2 * depth / 128, dtype="u64fx")
lamp = AreaLight(corner=(-1, depth, -1), edge_1=(2, 0, 0), edge_2=(0, 0, 2), normal=(0, -1, 0))

tracer = PhotonTracer().configure(volume, grid, lamp, primitives, linear_bvh)
labels = tracer.set_regions()                                # label m: medium m; the last label: outside the mesh
tracer.run_batches(n, batches, seed=1, labels=True)
totals, err = tracer.region_totals(), tracer.region_totals_error()
doses = np.array([1e-3, 1e-2, 1e-1]) * totals["peak"].max()  # D: fractions of the hottest voxel of the scene
dvh = tracer.dose_volume(doses)
names = ["cavity", "cone", "outside"]
print("%d photons in %d batches, %s voxels" % (n, batches, "x".join(map(str, grid.shape))))
for k, name in enumerate(names):
    if totals["voxels"][k] == 0:
        print("%-8s no voxel centre" % name)
        continue
    print("%-8s %8d voxels, absorbed %.4f of the launched weight +- %.2f %%, peak %.4g at (%.2f, %.2f, %.2f)"
          % ((name, totals["voxels"][k], totals["share"][k], 100 * err[k], totals["peak"][k]) + tuple(totals["peak_position"][k])))
    print("         V(>= D) for D = %s of the scene's peak: %s of its volume, %s of its weight"
          % ("/".join("%g" % f for f in (1e-3, 1e-2, 1e-1)), "/".join("%.2f %%" % (100 * v) for v in dvh["volume"][k]),
             "/".join("%.1f %%" % (100 * v) for v in dvh["weight"][k])))
