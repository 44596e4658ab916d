#!/usr/bin/env python3
"""The response of a slab to beams of finite width from ONE pencil-beam run: the traced tally is the medium's response G(x, y, z)
to a pencil, and the response to a beam of profile S(x, y) is G convolved with S in x and y -- taken on the device, for a 1 mm
and a 3 mm Gaussian and a flat-top beam, without tracing anything again.

    python examples/finite_beam.py [n_photons]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from light_transport_amd.src.beam_profiles import FlatTopProfile, GaussianProfile
from light_transport_amd.src.photon_tracing import LayeredSlab, OpticalMedium, PencilBeam, PhotonTracer, VoxelGrid

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10 ** 6
tissue = OpticalMedium(mu_a=0.1, mu_s=10.0, g=0.9, ior=1.0)                  # per mm: the medium of C2
grid = VoxelGrid((64, 64, 64), origin=(-12.8, -12.8, 0.0), voxel=0.4, dtype="u64fx")          # mm
pencil = PencilBeam((0.2, 0.2, 0.0), (0, 0, 1))                               # the centre of column (32, 32): the taps are centred on a column
tracer = PhotonTracer().configure(LayeredSlab([tissue], [np.inf]), grid, pencil)
tracer.run(n, seed=0)

beams = [("pencil", None), ("Gaussian, 1/e^2 radius 1 mm", GaussianProfile(1.0)), ("Gaussian, 1/e^2 radius 3 mm", GaussianProfile(3.0)),
         ("flat-top, radius 2 mm", FlatTopProfile(2.0))]
z = grid.origin[2] + (np.arange(grid.shape[2]) + 0.5) * grid.voxel[2]
rows = (0, 1, 2, 5, 10, 20, 50)
dv = grid.voxel_volume
print("%d photons traced once; absorbed energy density on the beam's axis per unit of beam power [1 / mm^3]" % n)
print("  %-30s" % "z [mm]" + "".join("%11.2f" % z[k] for k in rows))
for name, profile in beams:
    if profile is None:
        axis = tracer.absorbed()[:, 32, 32]                                   # the pencil's own column, read from the grid
    else:
        axis = tracer.beam_profile_at(profile)[:, 0]                          # [nz, 1]: a few KiB, no grid in between
    print("  %-30s" % name + "".join("%11.3e" % (axis[k] / (n * dv)) for k in rows))

# the whole response, where it is wanted: a few planes of it, or all of them
wide = GaussianProfile(3.0)
top = tracer.beam_response(wide, z_range=(0, 4))                              # [4, ny, nx]
whole = tracer.beam_response(wide)
assert np.array_equal(top, whole[:4])
lost = 1.0 - whole.sum() / ((1.0 - wide.cut_off()) * tracer.depth_profile().sum())
print("3 mm Gaussian: %.2e of the beam's power lies outside the taps, %.2e of the response beyond the grid's edge" % (wide.cut_off(), lost))
