#!/usr/bin/env python3
"""Absorbed weight against depth, A(z), and the cylindrical map A(r, z) of the slab of examples/photon_slab.py -- summed on
the device: a few KiB come back to the host, the 128 MiB grid never does.

    python examples/depth_profile.py [n_photons]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from light_transport_amd.src.photon_tracing import LayeredSlab, OpticalMedium, PencilBeam, PhotonTracer, VoxelGrid

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10 ** 7
tissue = OpticalMedium(mu_a=0.1, mu_s=10.0, g=0.9, ior=1.0)                 # per mm
grid = VoxelGrid((256, 256, 256), origin=(-12.8, -12.8, 0.0), voxel=0.1)     # mm
tracer = PhotonTracer().configure(LayeredSlab([tissue], [np.inf]), grid, PencilBeam((0, 0, 0), (0, 0, 1)))
tracer.run(n, seed=0)

a_z = tracer.depth_profile() / n                                             # [nz]: fraction of the launched weight per layer of voxels
a_rz, r_edges = tracer.rz_map((0.0, 0.0), dr=0.1, nr=100)                    # [nz, 101]: rings of 0.1 mm, the last column = beyond 10 mm
a_rz /= n
z = grid.origin[2] + (np.arange(grid.shape[2]) + 0.5) * grid.voxel[2]
print("%d photons; absorbed inside the grid: %.4f of the launched weight (counters: %.4f)"
      % (n, a_z.sum(), tracer.counters()["w_absorbed"] / n))
print("  z [mm]    A(z) per mm   A(r < 0.1, z)   A(1.0 <= r < 1.1, z)   A(r >= 10, z)")
for k in (0, 1, 2, 5, 10, 20, 50, 100, 200):
    print("  %6.2f   %11.4e   %13.4e   %20.4e   %13.4e" % (z[k], a_z[k] / grid.voxel[2], a_rz[k, 0], a_rz[k, 10], a_rz[k, 100]))
assert abs(a_rz.sum() - a_z.sum()) <= 1e-9 * a_z.sum()                       # the overflow ring keeps the map's total the grid's
