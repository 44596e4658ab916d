"""Volumetric photon transport -- the slot the reference left empty.

``src/photon_tracing.py`` of the reference is a 0-byte file and the medium
interaction of its walk is a TODO (bdpt.py:40).  This module fills the slot in
the reference's style -- configure plain objects, make ONE call, get a NumPy
array back, like ``render_scene(scene, primitives, bvh)``
(path_tracing_fix1.py:139-169):

    slab  = LayeredSlab([OpticalMedium(0.1, 10.0, 0.9, 1.0)], [np.inf])
    grid  = VoxelGrid((256, 256, 256), origin=(-12.8, -12.8, 0.0), voxel=(0.1,) * 3)
    dose  = trace_photons(slab, None, None, 10_000_000, seed=0, grid=grid,
                          source=PencilBeam((0, 0, 0), (0, 0, 1)))

The walk itself (hop / drop / spin) runs in the HIP kernels
behind include/lt.h; nothing here computes on the host.
"""
import math

import numpy as np

from .. import _lib
from .bvh_new import linear_bvh_arrays, triangles_array


class OpticalMedium:
    """mu_a, mu_s in 1/length; g = Henyey-Greenstein anisotropy; ior as Material.ior."""

    def __init__(self, mu_a, mu_s, g, ior=1.0):
        self.mu_a, self.mu_s, self.g, self.ior = float(mu_a), float(mu_s), float(g), float(ior)

    def as_tuple(self):
        return (self.mu_a, self.mu_s, self.g, self.ior)

    def __repr__(self):
        return "OpticalMedium(mu_a=%g, mu_s=%g, g=%g, ior=%g)" % self.as_tuple()


class LayeredSlab:
    """Plane-parallel layers stacked along +z from ``z0``; the last thickness may be inf."""

    def __init__(self, media, thicknesses, z0=0.0, n_above=1.0, n_below=1.0):
        if len(media) != len(thicknesses) or not media:
            raise ValueError("LayeredSlab: one thickness per medium, at least one layer")
        self.media = list(media)
        self.z_bounds = np.concatenate([[float(z0)], float(z0) + np.cumsum(np.asarray(thicknesses, dtype=np.float64))])
        self.n_above, self.n_below = float(n_above), float(n_below)


class MeshVolume:
    """Media bounded by triangles.  ``media``: list of OpticalMedium; every
    primitive carries ``med_front`` / ``med_back`` (medium index on the +normal /
    -normal side, -1 = exterior) -- see ``set_triangle_media``."""

    def __init__(self, media, start_medium=0):
        self.media = list(media)
        self.start_medium = int(start_medium)


def set_triangle_media(primitives, front, back):
    for p in primitives:
        p.med_front, p.med_back = int(front), int(back)
    return primitives


class VoxelGrid:
    """Tally of absorbed photon weight: shape (nx, ny, nz), C-order [nz][ny][nx]."""

    def __init__(self, shape, origin, voxel, dtype="f64"):
        self.shape = tuple(int(s) for s in shape)
        self.origin = tuple(float(o) for o in origin)
        self.voxel = tuple(float(v) for v in (voxel if np.ndim(voxel) else (voxel,) * 3))
        self.dtype = dtype

    @property
    def voxel_volume(self):
        return self.voxel[0] * self.voxel[1] * self.voxel[2]


class PencilBeam:
    def __init__(self, position, direction):
        self.position, self.direction = tuple(map(float, position)), tuple(map(float, direction))


class AreaLight:
    """Parallelogram emitting cosine-weighted about ``normal`` (role of the two
    ``is_light`` triangles + ``sample_light``, light_samples.py:90-116)."""

    def __init__(self, corner, edge_1, edge_2, normal):
        self.corner, self.edge_1, self.edge_2 = (tuple(map(float, v)) for v in (corner, edge_1, edge_2))
        self.normal = tuple(map(float, normal))


def uniform_table(n_photons, steps, seed=0):
    """Table RNG in the reference's manner (scene.py:68-69): uniforms drawn up
    front by NumPy's legacy MT19937 and addressed by (photon, step)."""
    return np.random.RandomState(seed).rand(int(n_photons), int(steps), 4)


def _box_key(lo, size, bin=(1, 1, 1)):
    """(lo, size, bin) as three tuples of three ints in x, y, z order: what Context.tally_box takes, hashable."""
    return tuple(_lib._int_triple(v, name) for v, name in ((lo, "lo"), (size, "size"), (bin, "bin")))


def block_lengths(size, bin):
    """int64 [ceil(size / bin)]: the voxels along one axis in every block of a box of ``size`` voxels binned by ``bin`` -- bin,
    but for the last one, which is clipped to the box."""
    if size < 1 or bin < 1:
        raise ValueError("size = %d and bin = %d have to be >= 1" % (size, bin))
    start = np.arange(0, size, bin, dtype=np.int64)
    return np.minimum(start + bin, size) - start


# label_volume sends one ray per voxel centre along this direction and reads the centre's medium off the nearest hit.  Near (0.3,
# 0.5, 0.81): parallel to no axis, no face diagonal and no space diagonal.  The components are (1 / pi, 1 / 2, 1 / sqrt(1.5)), whose
# ratios are irrational: voxel centres and mesh vertices usually sit on one rational lattice, and with a rational direction such
# as (0.3, 0.5, 0.81) itself whole families of rays meet a wall exactly ON the diagonal its two triangles share, where neither
# counts as hit (43 of 110 592 centres of the sphere-in-a-box scene came back without a hit that way).
LABEL_RAY_DIRECTION = np.array([1.0 / np.pi, 0.5, 1.0 / np.sqrt(1.5)]) / np.linalg.norm([1.0 / np.pi, 0.5, 1.0 / np.sqrt(1.5)])
LABEL_RAY_CHUNK = 1 << 22        # rays per intersect_rays call


def voxel_centres(grid, axis):
    """float64 [n]: the centres of the grid's voxels along axis 0 = x, 1 = y, 2 = z."""
    return grid.origin[axis] + grid.voxel[axis] * (np.arange(grid.shape[axis], dtype=np.float64) + 0.5)


def label_volume(ctx, geometry, grid):
    """uint8 [nz, ny, nx]: the medium every voxel CENTRE lies in, as Context.set_labels takes it.

    LayeredSlab (pure NumPy, ``ctx`` is not used): the layer k with z_bounds[k] <= z < z_bounds[k + 1] for the centre's z;
    LABEL_NONE (255) for centres outside every layer.  Labels 0 .. len(media) - 1.

    MeshVolume (the mesh has to be set on ``ctx``): one ray per voxel centre along LABEL_RAY_DIRECTION through
    Context.intersect_rays; the nearest hit decides by the walk's own rule -- with n the triangle's normal (ab x ac) and d
    the direction, d . n > 0 means the centre lies on the back side: med_back, otherwise med_front.  Medium m becomes label m;
    the exterior (-1) and rays that hit nothing become label len(media), "outside": len(media) + 1 labels.

    Two limits: the mesh has to be closed and consistently labelled (both sides of every surface name the media that really lie
    there), or the nearest hit says nothing about the centre; and a voxel is classified by its centre alone -- a voxel the
    surface cuts through belongs wholly to one side."""
    nx, ny, nz = grid.shape
    if isinstance(geometry, LayeredSlab):
        zb = np.asarray(geometry.z_bounds, dtype=np.float64)
        k = np.searchsorted(zb, voxel_centres(grid, 2), side="right") - 1
        lab = np.where((k >= 0) & (k < len(geometry.media)), k, _lib.LABEL_NONE).astype(np.uint8)
        return np.ascontiguousarray(np.broadcast_to(lab[:, None, None], (nz, ny, nx)))
    if not isinstance(geometry, MeshVolume):
        raise TypeError("label_volume: geometry must be a LayeredSlab or a MeshVolume")
    mesh = getattr(ctx, "_mesh", None)
    if mesh is None:
        raise ValueError("label_volume: set the mesh on the context first (PhotonTracer.configure or Context.set_mesh)")
    verts, med_front, med_back = mesh
    n_media = len(geometry.media)
    if n_media + 1 > _lib.MAX_LABELS:
        raise ValueError("label_volume: %d media and the outside are more than %d labels" % (n_media, _lib.MAX_LABELS))
    normal = np.cross(verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0])
    back = normal @ LABEL_RAY_DIRECTION > 0.0            # per triangle: a ray along the direction meets it from behind
    side = np.where(back, med_back, med_front)
    out = np.empty(nx * ny * nz, dtype=np.uint8)
    xs, ys, zs = (voxel_centres(grid, a) for a in range(3))
    planes = max(1, LABEL_RAY_CHUNK // (nx * ny))
    for z0 in range(0, nz, planes):
        z1 = min(nz, z0 + planes)
        o = np.empty((z1 - z0, ny, nx, 3))
        o[..., 0], o[..., 1], o[..., 2] = xs[None, None, :], ys[None, :, None], zs[z0:z1, None, None]
        o = o.reshape(-1, 3)
        for r0 in range(0, o.shape[0], LABEL_RAY_CHUNK):         # (a single plane above the chunk size)
            part = o[r0:r0 + LABEL_RAY_CHUNK]
            prim, _ = ctx.intersect_rays(part, np.broadcast_to(LABEL_RAY_DIRECTION, part.shape))
            med = np.where(prim >= 0, side[np.maximum(prim, 0)], -1)
            out[z0 * ny * nx + r0:z0 * ny * nx + r0 + part.shape[0]] = np.where(med >= 0, med, n_media)
    return out.reshape(nz, ny, nx)


DEFAULT_MAX_STEPS = 1000000      # lt.h: the walk's hard cap


class PhotonTracer:
    """Owns one device context; ``configure`` once, ``run`` as often as needed
    (runs accumulate until ``reset``)."""

    def __init__(self, device_id=0, ctx=None):
        self.ctx = ctx or _lib.Context(device_id)
        self.grid = None
        self.geometry = self.source = None
        self.quantity = "absorbed"
        self.photons = 0          # traced since the last reset (the fluence normalisation)
        self._profiles = {}       # run_batches: keep mask -> [batches, sum of the per-batch sums, sum of their squares]
        self._regions = {}        # run_batches: (lo, size, bin) -> the same moments of a binned box
        self._label_moments = {}  # run_batches: "labels" -> the same moments of the per-label totals

    def configure(self, geometry, grid, source, primitives=None, linear_bvh=None, max_steps=None, quantity="absorbed"):
        ctx = self.ctx
        ctx.set_media([m.as_tuple() for m in geometry.media])
        start_medium = 0
        if isinstance(geometry, LayeredSlab):
            ctx.set_layers(geometry.z_bounds, np.arange(len(geometry.media), dtype=np.int32), geometry.n_above,
                           geometry.n_below)
        elif isinstance(geometry, MeshVolume):
            if primitives is None or linear_bvh is None:
                raise ValueError("MeshVolume needs primitives (BVH order) and linear_bvh")
            mf = np.array([getattr(p, "med_front", -1) for p in primitives], dtype=np.int32)
            mb = np.array([getattr(p, "med_back", -1) for p in primitives], dtype=np.int32)
            ctx.set_mesh(triangles_array(primitives), mf, mb, linear_bvh_arrays(linear_bvh))
            start_medium = geometry.start_medium
        else:
            raise TypeError("geometry must be a LayeredSlab or a MeshVolume")
        ctx.set_grid(grid.shape, grid.origin, grid.voxel, grid.dtype)
        if isinstance(source, PencilBeam):
            ctx.set_source(_lib.SRC_PENCIL, source.position, source.direction, None, start_medium)
        elif isinstance(source, AreaLight):
            ctx.set_source(_lib.SRC_COSINE_QUAD, source.corner, source.normal,
                           list(source.edge_1) + list(source.edge_2), start_medium)
        else:
            raise TypeError("source must be a PencilBeam or an AreaLight")
        # every per-call setting is (re)set here, so that a call's result never depends on what an earlier user of the
        # same context left behind (the function-style API shares one context per device)
        ctx.set_max_steps(DEFAULT_MAX_STEPS if max_steps is None else max_steps)
        ctx.set_tally_mode("auto", 0)
        ctx.set_overlap(0)
        ctx.set_launch_config(0, 0)
        ctx.set_vertex_capture(0)
        ctx.set_tally_quantity(quantity)     # "absorbed": weight absorbed per voxel; "fluence": w / mu_t per interaction
        self.grid, self.quantity, self.photons = grid, quantity, 0
        self.geometry, self.source = geometry, source
        self._profiles, self._regions, self._label_moments = {}, {}, {}
        return self

    def run(self, n_photons, seed=0, photon_offset=0, rng_table=None, f32_walk=False, wait=True):
        self.ctx.launch(n_photons, seed=seed, photon_offset=photon_offset, rng_table=rng_table, f32_walk=f32_walk)
        self.photons += int(n_photons)
        if wait:
            self.ctx.sync()
        return self

    def run_batches(self, n_photons, n_batches, seed=0, photon_offset=0, f32_walk=False, profiles=(), regions=(), labels=False):
        """``n_photons`` traced as ``n_batches`` consecutive id ranges of equal size, every one closed with a fold of the batch
        statistics (turned on here if they are off): the grid ends as run(n_photons) leaves it, and relative_error() /
        error_summary() say how far every voxel can be trusted.  ``profiles``: keep-strings as tally_sum takes them ("z": the
        depth profile); for each, the device sum is taken after every fold and the moments of the per-batch differences are
        kept on the host for profile_error() -- voxels of one batch are correlated, so the error of a sum does not follow
        from the per-voxel moments.  ``regions``: (lo, size, bin) triples as region() takes them; each box is read after every
        fold in the same way, for region_error() -- the error of coarse voxels.  ``labels``: the per-label totals
        (Context.tally_label_sums, by the label volume of set_regions) are taken after every fold too, for
        region_totals_error()."""
        n_photons, n_batches = int(n_photons), int(n_batches)
        if n_batches < 2 or n_photons % n_batches:
            raise ValueError("run_batches: n_batches = %d must be at least 2 and divide n_photons = %d (equal batches)" % (n_batches, n_photons))
        ctx = self.ctx
        raw = self.grid.dtype in ("u64fx", _lib.TALLY["u64fx"])
        # what is summed after every fold: (the moments' dict, its key, the device sum)
        sums = [(self._profiles, m, lambda m=m: ctx.tally_sum(m, raw=raw)) for m in (_lib.keep_mask(k) for k in profiles)]
        sums += [(self._regions, r, lambda r=r: ctx.tally_box(*r, raw=raw)) for r in (_box_key(*r) for r in regions)]
        if labels:
            sums.append((self._label_moments, "labels", lambda: ctx.tally_label_sums(raw=raw)["raw" if raw else "weight"]))
        if not ctx.stats_enabled():
            ctx.stats_enable(True)
            self._profiles.clear()
            self._regions.clear()
            self._label_moments.clear()
        last = []
        for moments, key, read in sums:      # where a sum stands before the first batch (zero, unless earlier batches were run)
            last.append(read())
            if key not in moments:
                moments[key] = [0, np.zeros(last[-1].shape), np.zeros(last[-1].shape)]
        per = n_photons // n_batches
        for b in range(n_batches):
            ctx.launch(per, seed=seed, photon_offset=int(photon_offset) + b * per, f32_walk=f32_walk)
            ctx.stats_fold()
            for i, (moments, key, read) in enumerate(sums):
                now = read()
                d = (now - last[i]).astype(np.float64) * 2.0 ** -40 if raw else now - last[i]
                mom = moments[key]
                mom[0] += 1
                mom[1] = mom[1] + d
                mom[2] = mom[2] + d * d
                last[i] = now
        self.photons += n_photons
        ctx.sync()
        return self

    def relative_error(self):
        """float64 [nz, ny, nx]: relative standard error of every voxel over the batches of run_batches (NaN where the voxel
        holds nothing; 1 where a single batch contributed)."""
        return self.ctx.stats_relerr()

    def error_summary(self, edges):
        """(voxels, weight) per class of relative error, [len(edges) + 2] each (Context.stats_summary): weight[0] is what
        the voxels below edges[0] hold, the last entry the empty voxels.  Taken on the device: no grid is read back."""
        return self.ctx.stats_summary(edges)

    def profile_error(self, keep):
        """The relative standard error of tally_sum(keep) over the batches (same shape), from the moments run_batches kept
        for a ``profiles`` entry: _lib.relative_error(batches, sum, sum of squares)."""
        m = _lib.keep_mask(keep)
        if m not in self._profiles:
            raise ValueError("profile_error(%r): run_batches(..., profiles=(%r,)) first" % (keep, keep))
        n, s1, s2 = self._profiles[m]
        return _lib.relative_error(n, s1, s2)

    def region_error(self, lo, size, bin=(1, 1, 1)):
        """The relative standard error of region(lo, size, bin) over the batches (same shape), from the moments run_batches
        kept for a ``regions`` entry: _lib.relative_error(batches, sum, sum of squares)."""
        key = _box_key(lo, size, bin)
        if key not in self._regions:
            raise ValueError("region_error%r: run_batches(..., regions=(%r,)) first" % (key, key))
        n, s1, s2 = self._regions[key]
        return _lib.relative_error(n, s1, s2)

    def reset(self):
        self.ctx.zero_tally()
        self.photons = 0
        self._profiles, self._regions, self._label_moments = {}, {}, {}

    def absorbed(self):
        """float64 [nz, ny, nx]: absorbed photon weight per voxel (configure(..., quantity="absorbed"))."""
        if self.quantity != "absorbed":
            raise ValueError("this tracer tallies %r: absorbed() needs configure(..., quantity='absorbed')" % self.quantity)
        return self.ctx.read_grid()

    def fluence(self):
        """float64 [nz, ny, nx]: fluence per launched photon (1 / area) -- the grid of a tracer configured with
        quantity="fluence", where every interaction adds w / mu_t to its voxel, divided by voxel volume x photons.
        Correct in heterogeneous media (two layers, a mesh of another medium) and in media that do not absorb
        (mu_a = 0), where absorbed / mu_a has no meaning.  Normalised tally, role of path_tracing_fix1.py:162-166."""
        if self.quantity != "fluence":
            raise ValueError("this tracer tallies %r: fluence() needs configure(..., quantity='fluence')" % self.quantity)
        if self.photons <= 0:
            raise ValueError("fluence(): nothing traced since the last reset")
        return self.ctx.read_grid() / (self.grid.voxel_volume * float(self.photons))

    # -- sums taken on the device: a few KiB come back instead of the grid ------------------------------------------
    def _normalised(self, weight, voxels):
        """quantity="absorbed": the summed weight; "fluence": the mean fluence over the ``voxels`` (a count, or an array of
        counts) that went into each bin -- sum / (voxels x voxel volume x photons), NaN for a bin without voxels."""
        if self.quantity != "fluence":
            return weight
        if self.photons <= 0:
            raise ValueError("nothing traced since the last reset")
        n = np.asarray(voxels, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return weight / (np.where(n > 0, n, np.nan) * (self.grid.voxel_volume * float(self.photons)))

    def depth_profile(self):
        """float64 [nz]: absorbed weight per z layer of voxels, absorbed().sum((1, 2)) -- or the mean fluence of the layer --
        summed on the device (Context.tally_sum)."""
        nx, ny, _ = self.grid.shape
        return self._normalised(self.ctx.tally_sum("z"), nx * ny)

    def projection(self, axis):
        """The grid summed along one axis -- "x", "y" or "z", or the axis number of the [nz, ny, nx] array (0 = z, 1 = y,
        2 = x), so that projection(a) is absorbed().sum(a): [ny, nx] along z, [nz, nx] along y, [nz, ny] along x.  For a
        fluence tracer the mean fluence along the axis."""
        name = axis if isinstance(axis, str) else {0: "z", 1: "y", 2: "x", -1: "x", -2: "y", -3: "z"}.get(axis)
        if name not in ("x", "y", "z"):
            raise ValueError("projection(): axis must be 'x', 'y', 'z' or 0, 1, 2 (z, y, x), not %r" % (axis,))
        return self._normalised(self.ctx.tally_sum("xyz".replace(name, "")), self.grid.shape["xyz".index(name)])

    def rz_map(self, centre_xy, dr, nr):
        """(map [nz, nr + 1], r_edges [nr + 2]): the grid summed over rings of width ``dr`` about the axis through
        ``centre_xy`` parallel to z.  Ring k holds the columns whose centre lies in [r_edges[k], r_edges[k + 1]); the last one,
        [nr dr, inf), collects the rest, so the map's total is the grid's.  Absorbed weight per ring and z, or the mean
        fluence over the ring's voxels (NaN where a ring holds no column)."""
        nx, ny, _ = self.grid.shape
        bins = _lib.radial_bins((nx, ny), self.grid.origin[:2], self.grid.voxel[:2], centre_xy, dr, nr)
        m = self.ctx.tally_sum_columns(bins, int(nr) + 1)
        edges = np.append(float(dr) * np.arange(int(nr) + 1), np.inf)
        return self._normalised(m, np.bincount(bins.ravel(), minlength=int(nr) + 1)[None, :]), edges

    # -- parts of the grid read on the device: boxes, slices, coarser voxels (Context.tally_box) --------------------------
    def region(self, lo, size, bin=(1, 1, 1)):
        """(array [oz, oy, ox], (z_edges, y_edges, x_edges)): the box of ``size`` voxels that starts at voxel ``lo`` (both x, y,
        z), every ``bin`` = (bx, by, bz) voxels summed into one on the device; the last block of an axis is clipped to the
        box.  Absorbed weight per output voxel, or the mean fluence over the voxels that went into it (the clipped count).
        The edges, o + 1 per axis, are in scene units: origin + voxel x index, the last one the box's end."""
        lo, size, bin = _box_key(lo, size, bin)
        lengths = [block_lengths(size[a], bin[a]) for a in range(3)]
        voxels = lengths[2][:, None, None] * lengths[1][None, :, None] * lengths[0][None, None, :]
        edges = tuple(self.grid.origin[a] + self.grid.voxel[a] * (lo[a] + np.append(0, np.cumsum(lengths[a]))) for a in (2, 1, 0))
        return self._normalised(self.ctx.tally_box(lo, size, bin), voxels), edges

    def slice(self, axis, index, bin=1):
        """The plane of voxels at ``index`` along ``axis`` ("x", "y", "z" or 0, 1, 2 = z, y, x, as projection names it): [nz,
        nx] for "y", [nz, ny] for "x", [ny, nx] for "z" -- not a sum along the axis, the plane itself.  ``bin``: an int, or one
        per axis of the plane in x, y, z order, to bin it within the plane (region)."""
        name = axis if isinstance(axis, str) else {0: "z", 1: "y", 2: "x", -1: "x", -2: "y", -3: "z"}.get(axis)
        if name not in ("x", "y", "z"):
            raise ValueError("slice(): axis must be 'x', 'y', 'z' or 0, 1, 2 (z, y, x), not %r" % (axis,))
        a = "xyz".index(name)
        inplane = list(bin) if np.ndim(bin) else [bin, bin]
        if len(inplane) != 2:
            raise ValueError("slice(): bin=%r: an int or one per axis of the plane" % (bin,))
        lo, size, b3 = [0, 0, 0], list(self.grid.shape), inplane[:a] + [1] + inplane[a:]
        lo[a], size[a] = index, 1
        return np.squeeze(self.region(lo, size, b3)[0], axis=2 - a)

    def coarse(self, bin):
        """The whole grid at ``bin`` (an int, or (bx, by, bz)) times the voxel size: [ceil(nz / bz), ceil(ny / by), ceil(nx /
        bx)], the last voxel of an axis smaller where bin does not divide it (region)."""
        return self.region((0, 0, 0), self.grid.shape, bin if np.ndim(bin) else (bin,) * 3)[0]

    # -- results by region: a label volume, per-label totals and dose-volume histograms (Context.tally_label_sums) ---------
    def set_regions(self, labels=None):
        """Give every voxel a region.  Default: label_volume of the configured geometry -- the medium of every voxel centre (a
        mesh adds the label len(media), "outside").  An array uint8 [nz, ny, nx] (0 .. 63, or 255 to leave a voxel out) is taken
        as given.  configure() sets a new grid, which drops the labels.  Returns the label volume."""
        if labels is None:
            labels = label_volume(self.ctx, self.geometry, self.grid)
            n = len(self.geometry.media) + (1 if isinstance(self.geometry, MeshVolume) else 0)
            self.ctx.set_labels(labels, n)
        else:
            labels = np.asarray(labels)
            self.ctx.set_labels(labels)
        return labels

    def region_totals(self):
        """dict of arrays, one entry per label (the whole grid as label 0 without set_regions), taken on the device:
        ``weight`` the label's summed tally; ``share`` = weight / photons, the share of a launched photon's weight that went
        into it; ``total`` the sum in the units of absorbed(), or the mean fluence over the label's voxels; ``voxels`` and
        ``filled`` (non-zero voxels); ``peak`` its largest voxel in the units of absorbed() / fluence(); ``peak_index`` the lowest
        flat index that holds it (-1: the label has no voxel) and ``peak_position`` [n, 3] = (x, y, z) of that voxel's centre in
        scene units (NaN without a voxel)."""
        r = self.ctx.tally_label_sums()
        nx, ny, _ = self.grid.shape
        idx = r["peak_index"]
        cell = np.stack([idx % nx, (idx // nx) % ny, idx // (nx * ny)], axis=1).astype(np.float64)
        pos = np.asarray(self.grid.origin) + np.asarray(self.grid.voxel) * (cell + 0.5)
        pos[idx < 0] = np.nan
        share = r["weight"] / float(self.photons) if self.photons > 0 else np.full(idx.shape, np.nan)
        return dict(weight=r["weight"], share=share, total=self._normalised(r["weight"], r["voxels"]), voxels=r["voxels"],
                    filled=r["filled"], peak=self._normalised(r["peak"], 1), peak_index=idx, peak_position=pos)

    def dose_volume(self, edges):
        """dict(volume=..., weight=...), float64 [n_labels, len(edges)] each: per label the fraction of its voxels, and of its
        weight, in voxels AT OR ABOVE every edge -- the cumulative dose-volume histogram, from Context.tally_histogram.
        ``edges``: ascending, in the units of absorbed() / fluence().  NaN for a label without voxels (or without weight)."""
        e = np.asarray(edges, dtype=np.float64).reshape(-1)
        if self.quantity == "fluence":
            if self.photons <= 0:
                raise ValueError("nothing traced since the last reset")
            e = e * (self.grid.voxel_volume * float(self.photons))        # a voxel's fluence -> its weight
        vox, w = self.ctx.tally_histogram(e)
        above_v = vox[:, ::-1].cumsum(axis=1)[:, ::-1].astype(np.float64)
        above_w = w[:, ::-1].cumsum(axis=1)[:, ::-1]
        with np.errstate(divide="ignore", invalid="ignore"):
            return dict(volume=above_v[:, 1:] / np.where(above_v[:, :1] > 0, above_v[:, :1], np.nan),
                        weight=above_w[:, 1:] / np.where(above_w[:, :1] > 0, above_w[:, :1], np.nan))

    def region_totals_error(self):
        """The relative standard error of every label's total over the batches of run_batches(..., labels=True):
        _lib.relative_error(batches, sum, sum of squares) of the per-batch label totals."""
        if "labels" not in self._label_moments:
            raise ValueError("region_totals_error(): run_batches(..., labels=True) first")
        n, s1, s2 = self._label_moments["labels"]
        return _lib.relative_error(n, s1, s2)

    # -- the tally along rays: through a camera, along a line, along any direction (Context.tally_rays / tally_view) --------
    def _ray_quantity(self, what, threshold, call, dir_length):
        """One of "integral", "max", "depth" from the device call ``call(want, threshold as weight)`` -> dict of arrays, in this
        tracer's units.  integral: the tally's density integrated along the ray -- absorbed weight per volume x length, or
        fluence per launched photon x length; max: the largest voxel on the ray in the units of absorbed() / fluence(); depth:
        the geometric distance first_t x |d| from the ray's origin to where it enters the first voxel at or above ``threshold``
        (in those same units), inf where there is none."""
        if what not in ("integral", "max", "depth"):
            raise ValueError("what=%r: 'integral', 'max' or 'depth'" % (what,))
        if self.quantity == "fluence" and self.photons <= 0:
            raise ValueError("nothing traced since the last reset")
        per_voxel = self.grid.voxel_volume * (float(self.photons) if self.quantity == "fluence" else 1.0)
        if what == "integral":
            return call(("integral",), None)["integral"] / per_voxel
        if what == "max":
            return self._normalised(call(("max",), None)["max"], 1)
        if threshold is None or not np.isfinite(threshold) or threshold < 0:
            raise ValueError("what='depth' needs a finite threshold >= 0 in the units of absorbed() / fluence(), not %r" % (threshold,))
        as_weight = float(threshold) * (per_voxel if self.quantity == "fluence" else 1.0)       # a voxel's fluence -> its weight
        return call(("first",), as_weight)["first_t"] * dir_length

    def view(self, scene, what="integral", threshold=None):
        """float64 [H, W]: the tally seen through the camera of ``scene`` -- the pixel rays of render_scene (scene.camera[:3],
        scene.f_distance, np.linspace(left, right, W), np.linspace(top, bottom, H)), without their jitter, walked through the
        voxel grid on the device.  ``what``: "integral", "max" or "depth" (with ``threshold``), as _ray_quantity defines them."""
        xs = np.linspace(scene.left, scene.right, scene.width)
        ys = np.linspace(scene.top, scene.bottom, scene.height)
        cam = np.asarray(scene.camera, dtype=np.float64).ravel()[:3]
        length = np.linalg.norm(_lib.camera_rays(cam, scene.f_distance, xs, ys)[1], axis=-1)
        return self._ray_quantity(what, threshold, lambda want, thr: self.ctx.tally_view(cam, scene.f_distance, xs, ys, threshold=thr, want=want),
                                  length)

    def line_integral(self, p0, p1):
        """The tally's density integrated along the straight segment from ``p0`` to ``p1`` (a fibre, a biopsy track): a float in
        the units of view(..., "integral")."""
        p0, p1 = np.asarray(p0, dtype=np.float64).reshape(3), np.asarray(p1, dtype=np.float64).reshape(3)
        if not (np.all(np.isfinite(p0)) and np.all(np.isfinite(p1))) or np.array_equal(p0, p1):
            raise ValueError("line_integral: two distinct finite points, not %r and %r" % (p0.tolist(), p1.tolist()))
        call = lambda want, thr: self.ctx.tally_rays(p0[None, :], (p1 - p0)[None, :], t_range=(0.0, 1.0), threshold=thr, want=want)   # noqa: E731
        return float(self._ray_quantity("integral", None, call, 1.0)[0])

    def parallel_rays(self, direction, centre, up, width, height, extent):
        """(origins, dirs) float64 [height, width, 3] of parallel_projection: every ray runs along w = direction / |direction|.
        The image plane passes through ``centre``; with v = ``up`` made orthogonal to w and u = w x v (to the right of a viewer
        who looks along w with v up), pixel (i, j) sits at centre + a u + b v with a = ((j + 0.5) / width - 0.5) ew and b = (0.5 -
        (i + 0.5) / height) eh -- row 0 at the top -- where ``extent`` = (ew, eh), or one number for both, is the size of the image
        in scene units.  The rays start behind every corner of the grid."""
        w, c, v = (np.asarray(a, dtype=np.float64).reshape(3) for a in (direction, centre, up))
        width, height = int(width), int(height)
        ew, eh = (float(e) for e in (extent if np.ndim(extent) else (extent, extent)))
        if not np.all(np.isfinite(w)) or not np.any(w) or not np.all(np.isfinite(c)) or not np.all(np.isfinite(v)):
            raise ValueError("parallel_projection: direction, centre and up must be finite and direction non-zero")
        w = w / np.linalg.norm(w)
        v = v - np.dot(v, w) * w
        if not np.linalg.norm(v) > 1e-12 * max(np.linalg.norm(np.asarray(up, dtype=np.float64)), 1e-300):
            raise ValueError("parallel_projection: up=%r is parallel to the direction" % (up,))
        v = v / np.linalg.norm(v)
        u = np.cross(w, v)
        if width < 1 or height < 1 or not (ew > 0 and eh > 0 and np.isfinite(ew) and np.isfinite(eh)):
            raise ValueError("parallel_projection: width, height >= 1 and a finite extent > 0")
        lo = np.asarray(self.grid.origin)
        hi = lo + np.asarray(self.grid.voxel) * np.asarray(self.grid.shape)
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        back = float(np.min((corners - c) @ w)) - float(np.linalg.norm(hi - lo))
        a = ((np.arange(width) + 0.5) / width - 0.5) * ew
        b = (0.5 - (np.arange(height) + 0.5) / height) * eh
        o = c + a[None, :, None] * u + b[:, None, None] * v + back * w
        return np.ascontiguousarray(o), np.ascontiguousarray(np.broadcast_to(w, o.shape))

    def parallel_projection(self, direction, centre, up, width, height, extent, what="integral", threshold=None):
        """float64 [height, width]: the orthographic view of the tally along ``direction`` -- any direction, where projection()
        knows the three axes -- through the rays of parallel_rays; ``what`` as for view (a depth is measured from the rays'
        start behind the grid)."""
        o, d = self.parallel_rays(direction, centre, up, width, height, extent)
        call = lambda want, thr: self.ctx.tally_rays(o.reshape(-1, 3), d.reshape(-1, 3), threshold=thr, want=want)   # noqa: E731
        return self._ray_quantity(what, threshold, call, 1.0).reshape(o.shape[:2])

    # -- the response to a beam of finite width: the tally convolved in x and y on the device ------------------------
    def _beam_column(self, who):
        """(ix, iy) of the column whose centre the pencil enters through -- or ValueError: the convolution of the tally with a
        beam profile is the response to that beam only for a laterally invariant medium and taps centred on a column."""
        if not isinstance(self.geometry, LayeredSlab):
            raise ValueError("%s: needs a LayeredSlab (a laterally uniform medium), not %s" % (who, type(self.geometry).__name__))
        src = self.source
        if not isinstance(src, PencilBeam) or src.direction[0] != 0.0 or src.direction[1] != 0.0 or not src.direction[2] > 0.0:
            raise ValueError("%s: needs a PencilBeam along +z (a beam normal to the layers)" % who)
        col = []
        for axis in (0, 1):
            f = (src.position[axis] - self.grid.origin[axis]) / self.grid.voxel[axis]
            k = math.floor(f)
            if not abs(f - k - 0.5) <= 1e-6:
                raise ValueError("%s: the pencil has to enter at the centre of a column of voxels (within 1e-6 of a voxel); along %s it "
                                 "sits %.9g voxels from the column's edge" % (who, "xy"[axis], f - k))
            col.append(int(k))
        return tuple(col)

    def beam_response(self, profile, z_range=None):
        """float64 [nz_out, ny, nx]: the grid as a beam of ``profile`` (beam_profiles.GaussianProfile / FlatTopProfile, centred
        where the pencil is) would have left it -- the traced pencil-beam tally convolved in x and y with the profile's taps on
        the device (Context.tally_convolve), normalised exactly as absorbed() / fluence() normalise.  One run serves any number
        of beam sizes.  ``z_range`` = (z0, nz_out): those planes only.
        ValueError unless the geometry is a LayeredSlab, the source a PencilBeam along +z, and the pencil within 1e-6 of a
        voxel of a column's centre: only then is the convolution the response to the beam.  A grid too narrow for the pencil
        response plus the beam loses weight at its edges."""
        self._beam_column("beam_response")
        return self._beam_normalised(self.ctx.tally_convolve(profile.taps(self.grid.voxel[:2]), z_range))

    def beam_profile_at(self, profile, columns=None):
        """float64 [nz, n]: beam_response(profile) at the listed (ix, iy) columns only, for every z, without a grid in between
        (Context.tally_convolve_at).  Default: the source's own column, so that [:, 0] is the depth profile on the axis of the
        finite beam.  Refusals as for beam_response; at most 63 taps along an axis (Gaussian beams too: the taps go to the
        device as their outer product)."""
        col = self._beam_column("beam_profile_at")
        if columns is None:
            nx, ny, _ = self.grid.shape
            if not (0 <= col[0] < nx and 0 <= col[1] < ny):
                raise ValueError("beam_profile_at: the pencil's column %s lies outside the grid" % (col,))
            columns = np.array([col], dtype=np.int32)
        taps = profile.taps(self.grid.voxel[:2])
        if isinstance(taps, tuple) and max(len(t) for t in taps) > 63:
            raise ValueError("beam_profile_at: %d taps along an axis, lt_tally_convolve_at takes 63 (the separable form behind "
                             "beam_response takes 255)" % max(len(t) for t in taps))
        return self._beam_normalised(self.ctx.tally_convolve_at(taps, columns))

    def _beam_normalised(self, weight):
        if self.quantity != "fluence":
            return weight
        if self.photons <= 0:
            raise ValueError("nothing traced since the last reset")
        return weight / (self.grid.voxel_volume * float(self.photons))

    def absorbed_raw(self):
        return self.ctx.read_grid_raw()

    def counters(self):
        return self.ctx.read_counters()

    def kernel_ms(self):
        return self.ctx.last_kernel_ms()


def generate_light_subpaths(tracer, n_photons, max_depth, seed=0, photon_offset=0, as_objects=False):
    """Role of generate_light_subpaths (bdpt.py:258-268): trace ``n_photons`` from the configured source and return
    the first ``max_depth`` vertices of every path.  Returns (records [n, max_depth], counts [n]); with
    ``as_objects`` a list of lists of ``Vertex``.  The grid tally is accumulated as in a normal run."""
    tracer.ctx.set_vertex_capture(max_depth)
    try:
        tracer.run(n_photons, seed=seed, photon_offset=photon_offset)
        rec, cnt = tracer.ctx.read_vertices(n_photons)
    finally:
        tracer.ctx.set_vertex_capture(0)
    if not as_objects:
        return rec, cnt
    from .vertex import Vertex
    out = []
    for i in range(int(n_photons)):
        m = int(cnt[i])
        out.append([Vertex.from_record(rec[i, k], rec[i, k - 1] if k > 0 else None, rec[i, k + 1] if k + 1 < m else None)
                    for k in range(m)])
    return out


def fluence(absorbed, geometry, grid, n_photons):
    """Host post-step for an ABSORBED-weight grid of a LayeredSlab whose layer planes lie on voxel boundaries (Appendix
    C.4): fluence = absorbed / (mu_a(layer of the voxel) * dV * N), NaN where mu_a = 0.  Anything else -- a mesh, a plane
    inside a voxel, a medium that does not absorb -- has no per-voxel mu_a: trace with quantity="fluence" instead, where
    the device tallies w / mu_t directly (PhotonTracer.fluence / trace_photons(..., quantity="fluence"))."""
    if not isinstance(geometry, LayeredSlab):
        raise TypeError("fluence(): a per-voxel mu_a exists for a LayeredSlab only; use quantity='fluence' for meshes")
    a = np.asarray(absorbed, dtype=np.float64)
    nz = a.shape[0]
    z_lo = grid.origin[2] + grid.voxel[2] * np.arange(nz)
    z_hi = z_lo + grid.voxel[2]
    mu_a = np.full(nz, np.nan)
    tol = 1e-9 * grid.voxel[2]
    for k, m in enumerate(geometry.media):
        inside = (z_lo >= geometry.z_bounds[k] - tol) & (z_hi <= geometry.z_bounds[k + 1] + tol)
        mu_a[inside] = m.mu_a
    straddle = ~np.isfinite(mu_a) & (z_hi > geometry.z_bounds[0] + tol) & (z_lo < geometry.z_bounds[-1] - tol)
    if straddle.any():
        raise ValueError("fluence(): a layer plane cuts through voxel row(s) %s; use quantity='fluence'" % np.flatnonzero(straddle)[:4])
    with np.errstate(divide="ignore", invalid="ignore"):
        out = a / (np.where(mu_a > 0, mu_a, np.nan)[:, None, None] * grid.voxel_volume * float(n_photons))
    return out


def trace_photons(geometry, primitives, linear_bvh, n_photons, seed=0, grid=None, source=None, rng_table=None,
                  f32_walk=False, max_steps=None, device_id=0, return_counters=False, quantity="absorbed"):
    """One call, one array back, float64 [nz, ny, nx]: absorbed weight per voxel, or -- quantity="fluence" -- the
    fluence per launched photon (every interaction adds w / mu_t on the device; correct in heterogeneous media)."""
    if grid is None or source is None:
        raise ValueError("trace_photons needs grid= and source=")
    tr = PhotonTracer(ctx=_lib.default_context(device_id))
    tr.configure(geometry, grid, source, primitives, linear_bvh, max_steps, quantity)
    tr.run(n_photons, seed=seed, rng_table=rng_table, f32_walk=f32_walk)
    out = tr.fluence() if quantity == "fluence" else tr.absorbed()
    return (out, tr.counters()) if return_counters else out
