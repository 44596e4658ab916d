#!/usr/bin/env python3
"""The Cornell-box + cone scene of examples/cornell_cone.py, and the dose seen through the camera that rendered it:
  1. render_scene (surface path tracer) -> image [H, W, 3];
  2. the volumetric photon walk in the same geometry, kept on the device (PhotonTracer);
  3. PhotonTracer.view(scene, ...): per pixel of the SAME Scene the absorbed-energy density integrated along the pixel's ray, the
     hottest voxel on it, and how far the ray travels before it meets a voxel at 10 % of the peak -- a few hundred KiB come back,
     the 16 MiB grid stays where it is;
  4. the same dose along a tilted track and in an orthographic view along a diagonal.

    python examples/dose_view.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from light_transport_amd.src import constants as K
from light_transport_amd.src.bvh_new import BoundedBox, LinearBVHNode, build_bvh, flatten_bvh
from light_transport_amd.src.cornell_box import get_cone, get_cornell_box, get_front_wall, get_light_quad
from light_transport_amd.src.light_samples import generate_area_light_samples
from light_transport_amd.src.material import Material
from light_transport_amd.src.path_tracing_fix1 import render_scene
from light_transport_amd.src.photon_tracing import AreaLight, MeshVolume, OpticalMedium, PhotonTracer, VoxelGrid, set_triangle_media
from light_transport_amd.src.scene import Scene

depth = 7.5

surface = Material(color=K.WHITE_2, shininess=30, reflection=0.1, ior=1.5210, transmission=1)
left = Material(color=K.RED, shininess=30, reflection=0.1, ior=1.5210, transmission=1)
right = Material(color=K.GREEN, shininess=30, reflection=0.1, ior=1.5210, transmission=1)
source = Material(color=K.WHITE, shininess=1, reflection=0.9, ior=1.5, emission=200)


def bvh_of(objects):
    boxes = [BoundedBox(o, i) for i, o in enumerate(objects)]
    root, boxes, ordered, total = build_bvh(objects, boxes, 0, len(boxes), [], 0)
    linear, _ = flatten_bvh([LinearBVHNode() for _ in range(total)], root, 0)
    return ordered, linear


# ---- 1. surface render
light_tris = get_light_quad(depth, source)
objects = get_cornell_box(depth, surface, left, right) + get_cone(K.GLASS_MAT) + light_tris
lights = generate_area_light_samples(light_tris[0], light_tris[1], source, 1000, 4)
primitives, linear_bvh = bvh_of(objects)
np.random.seed(0)
scene = Scene(camera=np.array([0, 0, depth + 0.5, 1.0]), lights=lights, width=150, height=150, max_depth=4,
              f_distance=depth, number_of_samples=12)
image = render_scene(scene, primitives, linear_bvh)
print("render_scene: image %s, mean %.4f, max %.4f" % (image.shape, image.mean(), image.max()))

# ---- 2. photon transport in the same geometry (closed cavity), the tally kept on the device
walls = set_triangle_media(get_cornell_box(depth, surface, left, right) + get_front_wall(depth, surface)
                           + get_light_quad(depth, source), front=0, back=-1)
cone = set_triangle_media(get_cone(K.GLASS_MAT), front=0, back=1)
primitives, linear_bvh = bvh_of(walls + cone)
volume = MeshVolume([OpticalMedium(0.1, 10.0, 0.9, 1.0), OpticalMedium(1.0, 5.0, 0.8, K.GLASS_MAT.ior)], start_medium=0)
grid = VoxelGrid((128, 128, 128), origin=(-depth,) * 3, voxel=2 * depth / 128, dtype="u64fx")
lamp = AreaLight(corner=(-1, depth, -1), edge_1=(2, 0, 0), edge_2=(0, 0, 2), normal=(0, -1, 0))
tracer = PhotonTracer().configure(volume, grid, lamp, primitives, linear_bvh)
tracer.run(2_000_000, seed=1)
c = tracer.counters()
print("photon walk: absorbed fraction %.3f, %.0f steps per photon" % (c["w_absorbed"] / 2e6, c["steps"] / 2e6))

# ---- 3. the dose through the camera of the render
column = tracer.view(scene)                       # [150, 150]: absorbed weight per volume, integrated along every pixel's ray
peak = tracer.view(scene, "max")                  # the hottest voxel each pixel looks through
reach = tracer.view(scene, "depth", threshold=0.1 * peak.max())
seen = np.isfinite(reach)
print("view: %d x %d pixels; line integral up to %.4g (centre pixel %.4g); hottest voxel %.4g"
      % (column.shape[1], column.shape[0], column.max(), column[75, 75], peak.max()))
print("view: %d pixels look at the 10 %% isodose; it begins %.2f .. %.2f from the camera" % (seen.sum(), reach[seen].min(), reach[seen].max()))

# ---- 4. a tilted track, and an orthographic view along a diagonal
track = tracer.line_integral((-3.0, depth, -2.0), (2.0, -depth, 1.5))
ortho = tracer.parallel_projection(direction=(1, -1, 1), centre=(0, 0, 0), up=(0, 1, 0), width=96, height=96, extent=3.0 * depth)
print("line integral along a tilted track from the ceiling to the floor: %.4g" % track)
print("parallel projection along (1, -1, 1): %s, up to %.4g, %d pixels beside the cavity" % (ortho.shape, ortho.max(), (ortho == 0).sum()))
