"""ctypes binding of liblt_hip.so (the C ABI declared in include/lt.h).

The product has no CPU fallback: if the shared library or a gfx950 device is
missing, every compute entry point raises ``LtError``.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LT_HIP_LIBRARY") or os.path.join(_HERE, "liblt_hip.so")   # override: A/B builds of the same ABI

TALLY = {"f32": 0, "f64": 1, "u64fx": 2}
TALLY_NP = {0: np.float32, 1: np.float64, 2: np.uint64}
FX_SCALE = 2.0 ** 40
LABEL_NONE = 255      # LT_LABEL_NONE: a voxel of the label volume that is left out of everything
MAX_LABELS = 64
SRC_PENCIL, SRC_COSINE_QUAD = 0, 1
FLAG_F32_WALK = 1
FN = dict(HG_PDF=0, HG_SAMPLE=1, ONB=2, DISK=3, COSINE_HEMI=4, REFLECT=5, BOUNDARY=6, SPIN=7, WALK_MATH=8, WALK_MATH_RAW=9,
          PLANE_REACH=10, HG_WALK=11)
_FN_SHAPE = {0: (2, 1), 1: (2, 1), 2: (3, 6), 3: (2, 2), 4: (8, 4), 5: (6, 3), 6: (8, 5), 7: (5, 3), 8: (1, 5), 9: (1, 3),
             10: (17, 2), 11: (14, 2)}

# every symbol include/lt.h declares (tests check the library exports them all)
SYMBOLS = [
    "lt_abi_version", "lt_create", "lt_destroy", "lt_last_error", "lt_set_media", "lt_set_layers", "lt_set_mesh",
    "lt_set_grid", "lt_set_source", "lt_set_max_steps", "lt_set_launch_config", "lt_launch", "lt_sync",
    "lt_last_kernel_ms", "lt_zero_tally", "lt_read_grid", "lt_read_grid_f64", "lt_read_counters",
    "lt_grid_device_ptr", "lt_counters_device_ptr", "lt_stream", "lt_reduce_grid", "lt_intersect_rays",
    "lt_triangle_intersect", "lt_intersect_bounds", "lt_eval", "lt_rng_raw", "lt_device_info",
    "lt_set_surface_materials", "lt_set_lights", "lt_render_surface", "lt_set_vertex_capture", "lt_read_vertices",
    "lt_set_tally_mode", "lt_last_log_stages", "lt_reserve_log", "lt_render_surface_old", "lt_set_overlap", "lt_last_log_hot_tiles",
    "lt_last_log_info", "lt_set_tally_quantity", "lt_set_tuning", "lt_mesh_accel_info", "lt_build_bvh",
    "lt_layer_records", "lt_tally_sum_axes", "lt_tally_sum_columns", "lt_radial_bins", "lt_write_grid",
    "lt_stats_enable", "lt_stats_fold", "lt_stats_batches", "lt_stats_read_m2", "lt_stats_read_relerr", "lt_stats_summary",
    "lt_tally_convolve", "lt_tally_convolve_sep", "lt_tally_convolve_at", "lt_tally_box",
    "lt_set_labels", "lt_labels_info", "lt_tally_label_sums", "lt_tally_histogram",
    "lt_tally_rays", "lt_tally_view",
]
_U64P = C.POINTER(C.c_uint64)
_DP = C.POINTER(C.c_double)
_I64P = C.POINTER(C.c_int64)
# prototypes of the lt_stats_*, lt_tally_convolve*, lt_tally_box, label and ray entry points (lt.h); every one returns int
PROTOTYPES = {
    "lt_tally_rays": [C.c_void_p, _DP, _DP, _DP, C.c_size_t, C.c_double, _DP, _DP, _I64P, _DP, _I64P],
    "lt_tally_view": [C.c_void_p, C.c_int, C.c_int, _DP, C.c_double, _DP, _DP, C.c_double, _DP, _DP, _I64P, _DP, _I64P],
    "lt_set_labels": [C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, C.c_int],
    "lt_labels_info": [C.c_void_p, C.POINTER(C.c_int)],
    "lt_tally_label_sums": [C.c_void_p, _DP, _U64P, _U64P, _U64P, _DP, C.POINTER(C.c_int64)],
    "lt_tally_histogram": [C.c_void_p, _DP, C.c_int, _U64P, _DP, _U64P],
    "lt_tally_box": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _DP, _U64P],
    "lt_tally_convolve": [C.c_void_p, _DP, C.c_int, C.c_int, C.c_int, C.c_int, _DP],
    "lt_tally_convolve_sep": [C.c_void_p, _DP, C.c_int, _DP, C.c_int, C.c_int, C.c_int, _DP],
    "lt_tally_convolve_at": [C.c_void_p, _DP, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, _DP],
    "lt_stats_enable": [C.c_void_p, C.c_int],
    "lt_stats_fold": [C.c_void_p],
    "lt_stats_batches": [C.c_void_p, _U64P],
    "lt_stats_read_m2": [C.c_void_p, C.POINTER(C.c_double), C.c_size_t],
    "lt_stats_read_relerr": [C.c_void_p, C.POINTER(C.c_double), C.c_size_t],
    "lt_stats_summary": [C.c_void_p, C.POINTER(C.c_double), C.c_int, _U64P, C.POINTER(C.c_double), _U64P],
}

# lt_vertex as a NumPy record (112 bytes, same layout as the C struct)
VERTEX_DTYPE = np.dtype([("point", "<f8", 3), ("direction", "<f8", 3), ("g_norm", "<f8", 3), ("throughput", "<f8"),
                         ("pdf_pos", "<f8"), ("pdf_dir", "<f8"), ("kind", "<i4"), ("medium", "<i4"), ("step", "<u4"),
                         ("pad_", "<u4")])
VERTEX_LIGHT, VERTEX_REFLECTIVE, VERTEX_TRANSMISSIVE, VERTEX_VOLUME = 5, 3, 4, 7


class LtError(RuntimeError):
    pass


NODE_DTYPE = np.dtype([("lo", "<f8", 3), ("hi", "<f8", 3), ("offset", "<i4"), ("n_prims", "<i4"), ("axis", "<i4"), ("pad_", "<i4")])   # lt_bvh_node


def build_bvh_arrays(verts, split_method=1):
    """lt_build_bvh (host C++, no device): verts [T, 3, 3] -> (order [T] int32: ordered_prims[i] = input triangle order[i],
    nodes: structured array of lt_bvh_node records in pre-order)."""
    v = _f64(verts).reshape(-1, 3, 3)
    T = v.shape[0]
    order = np.empty(T, dtype=np.int32)
    nodes = np.zeros(max(2 * T, 1), dtype=NODE_DTYPE)
    nn = C.c_int(0)
    rc = lib().lt_build_bvh(_dp(v), C.c_int(T), C.c_int(int(split_method)), _ip(order), nodes.ctypes.data_as(C.c_void_p),
                            C.c_int(len(nodes)), C.byref(nn))
    if rc:
        raise LtError("lt_build_bvh failed (%d): needs >= 1 triangle with finite vertices and split_method 0 or 1" % rc)
    return order, nodes[:nn.value]


def layer_records(media, z_bounds, medium_idx, quantity=0, f32=False):
    """lt_layer_records (host C++, no device): (media_table [M, 12], zb [L + 1], layer_records [L, 12]) in walk precision, as a
    layered slab's walk kernels get them (field order: lt.h)."""
    arr = (Medium * len(media))(*[Medium(*map(float, m)) for m in media])
    zb = _f64(z_bounds)
    mi = np.ascontiguousarray(medium_idx, dtype=np.int32)
    dt = np.float32 if f32 else np.float64
    m_out, z_out, r_out = np.zeros((len(media), 12), dt), np.zeros(zb.size, dt), np.zeros((mi.size, 12), dt)
    rc = lib().lt_layer_records(arr, C.c_int(len(media)), C.c_int(int(quantity)), _dp(zb), _ip(mi), C.c_int(mi.size), C.c_int(int(f32)),
                                m_out.ctypes.data_as(C.c_void_p), z_out.ctypes.data_as(C.c_void_p), r_out.ctypes.data_as(C.c_void_p))
    if rc:
        raise LtError("lt_layer_records failed (%d): needs len(z_bounds) == len(medium_idx) + 1 and medium indices inside the media" % rc)
    return m_out, z_out, r_out


_KEEP_BITS = {"x": 1, "y": 2, "z": 4}


def keep_mask(keep):
    """The keep_mask of lt_tally_sum_axes from a string of the kept axes out of "xyz" in any order ("" keeps none: the grid
    total) or from the mask itself (0..6); all three axes kept is the grid: read_grid."""
    if isinstance(keep, str):
        k = keep.lower()
        if any(ch not in _KEEP_BITS for ch in k) or len(set(k)) != len(k):
            raise ValueError("keep=%r: a string of distinct axes out of 'x', 'y', 'z'" % (keep,))
        m = sum(_KEEP_BITS[ch] for ch in k)
    elif isinstance(keep, (int, np.integer)) and not isinstance(keep, bool):
        m = int(keep)
    else:
        raise ValueError("keep=%r: a string of axes or a mask 0..6" % (keep,))
    if not 0 <= m <= 6:
        raise ValueError("keep=%r: at least one axis has to be summed (mask 0..6); the whole grid is read_grid()" % (keep,))
    return m


def kept_shape(mask, grid_shape):
    """Shape of tally_sum's result: the kept axes of grid_shape = (nz, ny, nx), in that order."""
    return tuple(n for n, bit in zip(grid_shape, (4, 2, 1)) if mask & bit)


def _int_triple(v, name):
    """``v`` as a tuple of three ints (x, y, z), or ValueError naming the argument."""
    try:
        t = tuple(v)
    except TypeError:
        t = ()
    if len(t) != 3 or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) for k in t):
        raise ValueError("%s=%r: three integers in x, y, z order" % (name, v))
    return tuple(int(k) for k in t)


def box_shape(size, bin=(1, 1, 1)):
    """Shape (oz, oy, ox) of tally_box's result: ceil(size / bin) per axis, ``size`` and ``bin`` in x, y, z order (the last
    block of an axis is clipped, a bin beyond the box gives one block)."""
    s, b = _int_triple(size, "size"), _int_triple(bin, "bin")
    if min(s) < 1 or min(b) < 1:
        raise ValueError("box_shape: size=%r and bin=%r have to be >= 1 along every axis" % (size, bin))
    return tuple(-(-s[a] // b[a]) for a in (2, 1, 0))


def radial_bins(shape_xy, origin_xy, voxel_xy, centre_xy, dr, nr):
    """lt_radial_bins (host C++, no device): int32 [ny, nx], the ring 0..nr-1 of width dr about centre_xy that every column's
    centre falls in, nr for everything beyond nr * dr -- the table Context.tally_sum_columns(bins, nr + 1) takes."""
    nx, ny = (int(v) for v in shape_xy)
    out = np.empty((max(ny, 0), max(nx, 0)), dtype=np.int32)
    pair = lambda v: (C.c_double * 2)(*[float(x) for x in v][:2])      # noqa: E731
    rc = lib().lt_radial_bins(C.c_int(nx), C.c_int(ny), pair(origin_xy), pair(voxel_xy), pair(centre_xy), C.c_double(float(dr)),
                              C.c_int(int(nr)), _ip(out))
    if rc:
        raise LtError("lt_radial_bins failed (%d): needs nx, ny >= 1, dr > 0 and nr >= 1" % rc)
    return out


def relative_error(n, s1, m2):
    """The estimator of lt.h in NumPy, every line one IEEE double operation per element: the relative standard error of the
    mean over ``n`` equal batches from the total ``s1`` and the sum ``m2`` of the squared batch contributions.  Arrays in, an
    array out; NaN where s1 == 0 (no estimate), 0 where rounding leaves q < 1."""
    n = np.float64(n)
    s1, m2 = np.asarray(s1, dtype=np.float64), np.asarray(m2, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (n * m2) / (s1 * s1)
        v = q - 1.0
        v = np.where(v < 0.0, 0.0, v)
        r = np.sqrt(v / (n - 1.0))
    return np.where(s1 == 0.0, np.nan, r)


RAY_WANTS = ("integral", "max", "first")


def ray_wants(want):
    """``want`` of tally_rays / tally_view as a tuple out of RAY_WANTS, in that order: one name or several, at least one."""
    names = (want,) if isinstance(want, str) else tuple(want)
    if not names or any(w not in RAY_WANTS for w in names):
        raise ValueError("want=%r: one or more of %s" % (want, ", ".join(RAY_WANTS)))
    return tuple(w for w in RAY_WANTS if w in names)


def camera_rays(camera, f_distance, xs, ys):
    """(origins, dirs) float64 [H, W, 3]: the rays of lt_tally_view built on the host -- pixel (i, j) starts at the camera with
    d = (xs[j] - o.x, ys[i] - o.y, f_distance - o.z), the primary ray of lt_render_surface without its jitter."""
    o = _f64(np.asarray(camera, dtype=np.float64).ravel()[:3])
    xs, ys = _f64(xs).reshape(-1), _f64(ys).reshape(-1)
    d = np.empty((ys.size, xs.size, 3), dtype=np.float64)
    d[..., 0] = (xs - o[0])[None, :]
    d[..., 1] = (ys - o[1])[:, None]
    d[..., 2] = np.float64(f_distance) - o[2]
    return np.ascontiguousarray(np.broadcast_to(o, d.shape)), d


class Medium(C.Structure):
    _fields_ = [("mu_a", C.c_double), ("mu_s", C.c_double), ("g", C.c_double), ("n", C.c_double)]


class BvhNode(C.Structure):
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3), ("offset", C.c_int32),
                ("n_prims", C.c_int32), ("axis", C.c_int32), ("pad_", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [("photons", C.c_uint64), ("steps", C.c_uint64)] + [
        (k, C.c_double) for k in ("w_absorbed", "w_lost_outside_grid", "w_escaped_top", "w_escaped_bottom",
                                  "w_escaped_mesh", "w_specular", "w_roulette_net", "w_capped")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SurfaceMaterial(C.Structure):
    _fields_ = [("diffuse", C.c_double * 3), ("emission", C.c_double), ("ior", C.c_double),
                ("transmission", C.c_double), ("is_diffuse", C.c_int32), ("is_mirror", C.c_int32),
                ("is_light", C.c_int32), ("pad_", C.c_int32)]


class PointLight(C.Structure):
    _fields_ = [("source", C.c_double * 3), ("normal", C.c_double * 3), ("radiance", C.c_double * 3),
                ("total_area", C.c_double)]


def pack_surface_materials(primitives):
    """lt_surface_material per primitive from the reference-style objects (Material + is_light)."""
    arr = (SurfaceMaterial * max(len(primitives), 1))()
    for i, p in enumerate(primitives):
        m = p.material
        arr[i].diffuse[:] = [float(x) for x in m.color.diffuse[:3]]
        arr[i].emission, arr[i].ior, arr[i].transmission = float(m.emission), float(m.ior), float(m.transmission)
        arr[i].is_diffuse, arr[i].is_mirror, arr[i].is_light = int(m.is_diffuse), int(m.is_mirror), int(p.is_light)
    return arr


def pack_lights(lights):
    """lt_point_light per Light sample (scene.py:12-17); radiance = emission * color.diffuse."""
    arr = (PointLight * max(len(lights), 1))()
    for i, l in enumerate(lights):
        arr[i].source[:] = [float(x) for x in l.source[:3]]
        arr[i].normal[:] = [float(x) for x in l.normal[:3]]
        arr[i].radiance[:] = [float(l.material.emission * x) for x in l.material.color.diffuse[:3]]
        arr[i].total_area = float(l.total_area)
    return arr


_lib = None


def build(verbose=False):
    """Compile liblt_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc")]
    if not verbose:
        cmd.append("-s")
    subprocess.check_call(cmd)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LtError("liblt_hip.so is not built (run light_transport_amd.build() or "
                          "`make -C light_transport_amd/csrc`); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.lt_last_error.restype = C.c_char_p
        L.lt_last_error.argtypes = [C.c_void_p]
        L.lt_stream.restype = C.c_void_p
        L.lt_stream.argtypes = [C.c_void_p]
        for name, argtypes in PROTOTYPES.items():
            f = getattr(L, name, None)      # (an older build of the ABI behind LT_HIP_LIBRARY: the call then fails by name)
            if f is not None:
                f.argtypes, f.restype = argtypes, C.c_int
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.reshape(shape) if shape is not None else a


def _conv_taps(a, ndim, name):
    """A tap array as the convolution calls take it: real numbers, ``ndim`` axes, not empty -> C-contiguous float64.  (What the
    values and counts may be is the library's to check.)"""
    t = np.asarray(a)
    if t.dtype.kind not in "fiu" or t.ndim != ndim or t.size == 0:
        raise LtError("%s: expected a non-empty %d-D array of real numbers, got %s %s" % (name, ndim, t.dtype.name, t.shape))
    return np.ascontiguousarray(t, dtype=np.float64)


class Context:
    """One lt_ctx: one GPU, one HIP stream, one voxel grid."""

    def __init__(self, device_id=0):
        self._h = C.c_void_p()
        rc = lib().lt_create(C.byref(self._h), C.c_int(device_id))
        if rc != 0:
            msg = lib().lt_last_error(None)
            raise LtError("lt_create failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        self.device_id = device_id
        self._grid_shape = None
        self._tally = None
        self._mesh = None

    # -- plumbing ---------------------------------------------------------
    def _ck(self, rc, what):
        if rc != 0:
            msg = lib().lt_last_error(self._h)
            raise LtError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().lt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- scene ------------------------------------------------------------
    def set_media(self, media):
        arr = (Medium * len(media))(*[Medium(*map(float, m)) for m in media])
        self._ck(lib().lt_set_media(self._h, arr, C.c_int(len(media))), "lt_set_media")

    def set_layers(self, z_bounds, medium_idx, n_above=1.0, n_below=1.0):
        zb = _f64(z_bounds)
        mi = np.ascontiguousarray(medium_idx, dtype=np.int32)
        if zb.size != mi.size + 1:
            raise LtError("set_layers: need len(z_bounds) == len(medium_idx) + 1")
        self._ck(lib().lt_set_layers(self._h, _dp(zb), _ip(mi), C.c_int(mi.size), C.c_double(n_above),
                                     C.c_double(n_below)), "lt_set_layers")

    def set_mesh(self, verts, med_front, med_back, nodes):
        """nodes: lt_bvh_node records -- a structured array (NODE_DTYPE, as build_bvh_arrays returns) or a dict of arrays
        lo [N, 3], hi [N, 3], offset, n_prims, axis (as linear_bvh_arrays returns)."""
        v = _f64(verts).reshape(-1, 3, 3)
        mf = np.ascontiguousarray(med_front, dtype=np.int32)
        mb = np.ascontiguousarray(med_back, dtype=np.int32)
        if isinstance(nodes, np.ndarray) and nodes.dtype == NODE_DTYPE:
            arr = np.ascontiguousarray(nodes)
        else:       # packed with array assignments: a per-node Python loop costs ~0.2 s on a 20 000-node tree
            n_ = len(nodes["offset"])
            arr = np.zeros(n_, dtype=NODE_DTYPE)
            arr["lo"] = np.asarray(nodes["lo"], dtype=np.float64).reshape(n_, 3); arr["hi"] = np.asarray(nodes["hi"], dtype=np.float64).reshape(n_, 3)
            arr["offset"] = nodes["offset"]; arr["n_prims"] = nodes["n_prims"]; arr["axis"] = nodes["axis"]
        n = len(arr)
        if mf.size != v.shape[0] or mb.size != v.shape[0]:
            raise LtError("set_mesh: medium arrays must have one entry per triangle")
        self._ck(lib().lt_set_mesh(self._h, _dp(v), _ip(mf), _ip(mb), C.c_int(v.shape[0]), arr.ctypes.data_as(C.c_void_p), C.c_int(n)),
                 "lt_set_mesh")
        self._mesh = (v.copy(), mf.copy(), mb.copy())      # host copy: photon_tracing.label_volume reads a hit's sides from it

    def set_grid(self, shape, origin, voxel, dtype="f64"):
        nx, ny, nz = (int(s) for s in shape)
        o = (C.c_double * 3)(*map(float, origin))
        vx = (C.c_double * 3)(*map(float, voxel))
        t = TALLY[dtype] if isinstance(dtype, str) else int(dtype)
        self._ck(lib().lt_set_grid(self._h, C.c_int(nx), C.c_int(ny), C.c_int(nz), o, vx, C.c_int(t)), "lt_set_grid")
        self._grid_shape = (nz, ny, nx)
        self._tally = t

    def set_source(self, type=SRC_PENCIL, pos=(0, 0, 0), dir=(0, 0, 1), extra=None, start_medium=0):
        p = (C.c_double * 3)(*map(float, pos))
        d = (C.c_double * 3)(*map(float, dir))
        ex = (C.c_double * 6)(*map(float, (list(extra) + [0.0] * 6)[:6])) if extra is not None else None
        self._ck(lib().lt_set_source(self._h, C.c_int(type), p, d, ex, C.c_int(start_medium)), "lt_set_source")

    def set_max_steps(self, n):
        self._ck(lib().lt_set_max_steps(self._h, C.c_uint32(int(n))), "lt_set_max_steps")

    def set_tally_quantity(self, quantity):
        """"absorbed" (default): an interaction adds the absorbed weight w mu_a / mu_t to its voxel; "fluence": it adds
        w / mu_t, so that grid / (voxel volume x photons) IS the fluence, in heterogeneous media too (lt.h)."""
        q = {"absorbed": 0, "fluence": 1}.get(quantity, quantity)
        self._ck(lib().lt_set_tally_quantity(self._h, C.c_int(int(q))), "lt_set_tally_quantity")

    def mesh_accel_info(self):
        """dict(kind, march_dims, march_entries, clearance_dims) of the current mesh (lt.h: lt_mesh_accel_info)."""
        kind, ent = C.c_int(0), C.c_uint64(0)
        md, cd = (C.c_int * 3)(), (C.c_int * 3)()
        self._ck(lib().lt_mesh_accel_info(self._h, C.byref(kind), md, C.byref(ent), cd), "lt_mesh_accel_info")
        return dict(kind=kind.value, march_dims=tuple(md), march_entries=ent.value, clearance_dims=tuple(cd))

    def set_tuning(self, key, value=-1):
        """An experiment knob of the library (lt.h: lt_set_tuning); value < 0 (default) restores the built-in default."""
        self._ck(lib().lt_set_tuning(self._h, key.encode(), C.c_int64(int(value))), "lt_set_tuning")

    def tuning(self, **knobs):
        """Context manager: the given knobs for the duration of the block, defaults restored afterwards."""
        ctx = self

        class _T:
            def __enter__(self_):
                for k, v in knobs.items():
                    ctx.set_tuning(k, v)
                return ctx

            def __exit__(self_, *a):
                for k in knobs:
                    ctx.set_tuning(k, -1)
        return _T()

    def set_launch_config(self, blocks_per_cu=0, threads_per_block=0):
        self._ck(lib().lt_set_launch_config(self._h, C.c_int(blocks_per_cu), C.c_int(threads_per_block)),
                 "lt_set_launch_config")

    def set_tally_mode(self, mode="auto", log_bytes=0):
        """'atomic': global atomics per deposit; 'log': deposit log + tile partition + LDS reduce;
        'auto' (default): log for layered slabs and f32 mesh walks, atomic for f64 mesh walks."""
        m = {"atomic": 0, "log": 1, "auto": 2}[mode] if isinstance(mode, str) else int(mode)
        self._ck(lib().lt_set_tally_mode(self._h, C.c_int(m), C.c_uint64(int(log_bytes))), "lt_set_tally_mode")

    def set_overlap(self, lanes=0):
        """Overlap inside one launch: 2 = sub-batches alternate between two streams of the ctx (one batch's log
        reduction runs beside the next batch's walk), 1 = one stream, 0 = auto (try both once, keep the faster)."""
        self._ck(lib().lt_set_overlap(self._h, C.c_int(int(lanes))), "lt_set_overlap")

    def last_log_info(self):
        """dict(records, overflow_records, batches, lanes) of the last log-mode launch, or None."""
        rec, ovf, bat, lanes = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        if lib().lt_last_log_info(self._h, C.byref(rec), C.byref(ovf), C.byref(bat), C.byref(lanes)) != 0:
            return None
        return dict(records=rec.value, overflow_records=ovf.value, batches=bat.value, lanes=lanes.value)

    def last_log_hot_tiles(self):
        """(hot tiles, pilot-count threshold) of the last log-mode launch: (0, 0) unless the hot-tile two-pass form ran."""
        h, t = C.c_uint32(), C.c_uint32()
        self._ck(lib().lt_last_log_hot_tiles(self._h, C.byref(h), C.byref(t)), "lt_last_log_hot_tiles")
        return h.value, t.value

    def reserve_log(self, n_photons):
        self._ck(lib().lt_reserve_log(self._h, C.c_uint64(int(n_photons))), "lt_reserve_log")

    # -- run --------------------------------------------------------------
    def launch(self, n_photons, seed=0, photon_offset=0, rng_table=None, f32_walk=False):
        tab, steps = None, 0
        if rng_table is not None:
            tab = _f64(rng_table)
            if tab.ndim != 3 or tab.shape[0] != n_photons or tab.shape[2] != 4:
                raise LtError("rng_table must have shape [n_photons, steps, 4]")
            steps = tab.shape[1]
        flags = FLAG_F32_WALK if f32_walk else 0
        self._captured_max_vertices = getattr(self, "_max_vertices", 0)
        self._ck(lib().lt_launch(self._h, C.c_uint64(int(n_photons)), C.c_uint64(int(photon_offset)),
                                 C.c_uint64(int(seed) & (2 ** 64 - 1)), _dp(tab), C.c_uint64(steps),
                                 C.c_uint32(flags)), "lt_launch")

    def sync(self):
        self._ck(lib().lt_sync(self._h), "lt_sync")

    def last_kernel_ms(self):
        ms = C.c_double()
        self._ck(lib().lt_last_kernel_ms(self._h, C.byref(ms)), "lt_last_kernel_ms")
        return ms.value

    def last_log_stages(self):
        """dict(walk_ms, scan_ms, partition_ms, reduce_ms, records, batches) of the last log-mode launch, or None."""
        ms = (C.c_double * 4)()
        rec, bat = C.c_uint64(), C.c_uint64()
        if lib().lt_last_log_stages(self._h, ms, C.byref(rec), C.byref(bat)) != 0:
            return None
        return dict(walk_ms=ms[0], scan_ms=ms[1], partition_ms=ms[2], reduce_ms=ms[3], records=rec.value, batches=bat.value)

    def zero_tally(self):
        self._ck(lib().lt_zero_tally(self._h), "lt_zero_tally")

    # -- readback ---------------------------------------------------------
    def read_grid_raw(self):
        out = np.empty(self._grid_shape, dtype=TALLY_NP[self._tally])
        self._ck(lib().lt_read_grid(self._h, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)), "lt_read_grid")
        return out

    def read_grid_into(self, buf):
        """Raw tally into a caller-owned contiguous buffer of exactly the grid's size in bytes (e.g. pinned host
        memory: the D2H copy then runs at the link's rate)."""
        a = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
        self._ck(lib().lt_read_grid(self._h, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)), "lt_read_grid")
        return buf

    def read_grid(self):
        """Absorbed weight per voxel as float64 [nz, ny, nx]."""
        out = np.empty(self._grid_shape, dtype=np.float64)
        self._ck(lib().lt_read_grid_f64(self._h, _dp(out), C.c_size_t(out.size)), "lt_read_grid_f64")
        return out

    def write_grid(self, array):
        """Overwrite the device grid with a raw tally [nz, ny, nx] of the dtype the grid was set with (what read_grid_raw
        returned); the counters stay as they are."""
        a = np.asarray(array)
        if self._grid_shape is not None and (a.dtype != np.dtype(TALLY_NP[self._tally]) or a.shape != self._grid_shape):
            raise LtError("write_grid: expected %s %s, got %s %s" % (np.dtype(TALLY_NP[self._tally]).name, self._grid_shape,
                                                                     a.dtype.name, a.shape))
        a = np.ascontiguousarray(a)
        self._ck(lib().lt_write_grid(self._h, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)), "lt_write_grid")

    def _sum_buffers(self, shape, raw):
        out = np.empty(shape, dtype=np.float64)
        rawbuf = np.empty(shape, dtype=np.uint64) if raw else None
        return out, rawbuf, (rawbuf.ctypes.data_as(C.POINTER(C.c_uint64)) if raw else None)

    def tally_sum(self, keep, raw=False):
        """The grid summed on the device over the axes not in ``keep`` ("", "x", "y", "z", "xy", "xz", "yz" in any letter
        order, or the mask: 1 = x, 2 = y, 4 = z): float64 weight shaped by the kept axes in (z, y, x) order -- "z" is the
        depth profile [nz], "" the grid total (0-d).  raw=True (u64 fixed-point tally only): the exact uint64 sums."""
        m = keep_mask(keep)
        out, rawbuf, rp = self._sum_buffers(kept_shape(m, self._grid_shape or (0, 0, 0)), raw)
        self._ck(lib().lt_tally_sum_axes(self._h, C.c_int(m), _dp(out), rp), "lt_tally_sum_axes")
        return rawbuf if raw else out

    def tally_sum_columns(self, bins, n_bins, raw=False):
        """[nz, n_bins]: for every z the sum of the voxels whose (y, x) column carries that bin.  ``bins``: int [ny, nx],
        0..n_bins-1 or -1 to leave a column out (radial_bins gives the table of an r-z map).  raw as in tally_sum."""
        b = np.ascontiguousarray(bins, dtype=np.int32)
        nz, ny, nx = self._grid_shape or (0, 0, 0)
        if self._grid_shape is not None and b.shape != (ny, nx):
            raise LtError("tally_sum_columns: bins must have shape (ny, nx) = %s, got %s" % ((ny, nx), b.shape))
        out, rawbuf, rp = self._sum_buffers((nz, max(int(n_bins), 0)), raw)
        self._ck(lib().lt_tally_sum_columns(self._h, _ip(b), C.c_int(int(n_bins)), _dp(out), rp), "lt_tally_sum_columns")
        return rawbuf if raw else out

    def tally_box(self, lo, size, bin=(1, 1, 1), raw=False):
        """[oz, oy, ox] = box_shape(size, bin): the box of ``size`` voxels whose first voxel is ``lo`` (both x, y, z), every
        ``bin`` = (bx, by, bz) grid voxels of it summed into one output voxel on the device; the last block of an axis is
        clipped to the box.  bin (1, 1, 1): the sub-volume itself -- one voxel thick, a slice.  float64 weight; raw=True (u64
        fixed-point tally only): the exact uint64 sums.  A box that leaves the grid: LtError."""
        lo3, s3, b3 = _int_triple(lo, "lo"), _int_triple(size, "size"), _int_triple(bin, "bin")
        big = [v for v in lo3 + s3 + b3 if not -2 ** 31 <= v < 2 ** 31]
        if big:
            raise ValueError("tally_box: %d does not fit an int32" % big[0])
        shape = box_shape(s3, b3) if min(s3) >= 1 and min(b3) >= 1 else (0, 0, 0)       # (the library names what is wrong)
        out, rawbuf, rp = self._sum_buffers(shape, raw)
        arr = [(C.c_int32 * 3)(*v) for v in (lo3, s3, b3)]
        self._ck(lib().lt_tally_box(self._h, arr[0], arr[1], arr[2], _dp(out), rp), "lt_tally_box")
        return rawbuf if raw else out

    # -- the tally convolved in x and y (lt.h: lt_tally_convolve*) --------------------------------------------------------
    def tally_convolve(self, taps, z_range=None):
        """float64 [nz_out, ny, nx]: the tally as weight, every plane convolved in x and y with ``taps`` -- a 2-D float64 array
        [kh, kw] (odd counts up to 63), or a pair (taps_x, taps_y) of 1-D arrays (odd counts up to 255) for the separable
        form, two 1-D passes.  Taps are finite and >= 0; weight from beyond the grid's edge is missing.  ``z_range`` = (z0,
        nz_out): those planes only (default: all)."""
        nz, ny, nx = self._grid_shape or (0, 0, 0)
        z0, nz_out = (0, nz) if z_range is None else (int(z_range[0]), int(z_range[1]))
        if self._grid_shape is not None and (z0 < 0 or nz_out < 1 or z0 + nz_out > nz):
            raise LtError("tally_convolve: z_range = (z0, nz_out) = (%d, %d) does not lie inside 0 .. %d" % (z0, nz_out, nz))
        out = np.empty((max(nz_out, 0), ny, nx), dtype=np.float64)
        if isinstance(taps, (tuple, list)) and len(taps) == 2 and np.ndim(taps[0]) == 1 and np.ndim(taps[1]) == 1:
            tx, ty = _conv_taps(taps[0], 1, "taps_x"), _conv_taps(taps[1], 1, "taps_y")
            self._ck(lib().lt_tally_convolve_sep(self._h, _dp(tx), tx.size, _dp(ty), ty.size, z0, nz_out, _dp(out)), "lt_tally_convolve_sep")
        else:
            t = _conv_taps(taps, 2, "taps")
            self._ck(lib().lt_tally_convolve(self._h, _dp(t), t.shape[0], t.shape[1], z0, nz_out, _dp(out)), "lt_tally_convolve")
        return out

    def tally_convolve_at(self, taps, columns):
        """float64 [nz, n]: the convolved tally at the listed columns only, for every z.  ``taps``: 2-D [kh, kw], or a pair
        (taps_x, taps_y), which is turned into its outer product; ``columns``: int [n, 2] of (ix, iy) inside the grid, n up to
        4096."""
        if isinstance(taps, (tuple, list)) and len(taps) == 2 and np.ndim(taps[0]) == 1 and np.ndim(taps[1]) == 1:
            taps = np.outer(_conv_taps(taps[1], 1, "taps_y"), _conv_taps(taps[0], 1, "taps_x"))
        t = _conv_taps(taps, 2, "taps")
        cols = np.asarray(columns)
        if cols.dtype.kind not in "iu" or cols.ndim != 2 or cols.shape[1] != 2 or cols.shape[0] < 1:
            raise LtError("tally_convolve_at: columns must be an integer array [n, 2] of (ix, iy), n >= 1; got %s %s" % (cols.dtype.name, cols.shape))
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        nz = (self._grid_shape or (0, 0, 0))[0]
        out = np.empty((nz, cols.shape[0]), dtype=np.float64)
        self._ck(lib().lt_tally_convolve_at(self._h, _dp(t), t.shape[0], t.shape[1], _ip(cols), cols.shape[0], _dp(out)), "lt_tally_convolve_at")
        return out

    # -- statistical error of the tally from batch moments (lt.h: lt_stats_*) ------------------------------------------
    def stats_enable(self, on=True):
        """Turn the batch statistics on (two more device buffers of the grid's extent, zeroed; needs a grid nothing was
        launched into or written to since set_grid / zero_tally) or off."""
        self._ck(lib().lt_stats_enable(self._h, int(bool(on))), "lt_stats_enable")

    def stats_fold(self):
        """Close a batch (async): what the grid gained since the last fold goes, squared, into the second moments."""
        self._ck(lib().lt_stats_fold(self._h), "lt_stats_fold")

    def stats_enabled(self):
        """Whether the batch statistics are on (set_grid turns them off)."""
        return lib().lt_stats_batches(self._h, C.byref(C.c_uint64())) == 0

    def stats_batches(self):
        """Batches closed since the statistics were turned on or the tally was zeroed."""
        n = C.c_uint64()
        self._ck(lib().lt_stats_batches(self._h, C.byref(n)), "lt_stats_batches")
        return n.value

    def stats_m2(self):
        """float64 [nz, ny, nx]: the sum over the closed batches of the squared batch contribution."""
        out = np.empty(self._grid_shape or (0, 0, 0), dtype=np.float64)
        self._ck(lib().lt_stats_read_m2(self._h, _dp(out), out.size), "lt_stats_read_m2")
        return out

    def stats_relerr(self):
        """float64 [nz, ny, nx]: the relative standard error of every voxel (relative_error), NaN where it holds nothing."""
        out = np.empty(self._grid_shape or (0, 0, 0), dtype=np.float64)
        self._ck(lib().lt_stats_read_relerr(self._h, _dp(out), out.size), "lt_stats_read_relerr")
        return out

    def stats_summary(self, edges, raw=False):
        """(voxels uint64, weight) per error class, [len(edges) + 2] each: class k = the voxels whose relative error has k of
        the ascending ``edges`` at or below it, the last entry the voxels that hold nothing.  raw=True (u64 fixed-point tally
        only): weight is the exact uint64 sums."""
        e = _f64(edges).reshape(-1)
        vox = np.zeros(e.size + 2, dtype=np.uint64)
        out, rawbuf, rp = self._sum_buffers((e.size + 2,), raw)
        self._ck(lib().lt_stats_summary(self._h, _dp(e), int(e.size), vox.ctypes.data_as(_U64P), _dp(out), rp), "lt_stats_summary")
        return vox, (rawbuf if raw else out)

    # -- the tally by region: label volume, per-label totals, histograms (lt.h: lt_set_labels ...) -------------------------
    def set_labels(self, labels, n_labels=None):
        """The label volume of the grid: uint8 [nz, ny, nx], every voxel 0 .. n_labels - 1 or LABEL_NONE (255: left out of
        everything); n_labels (1 .. 64) defaults to the largest label + 1.  None releases it: the whole grid is label 0 again.
        set_grid drops the labels."""
        if labels is None:
            self._ck(lib().lt_set_labels(self._h, None, 0, 0), "lt_set_labels")
            return
        a = np.asarray(labels)
        if a.dtype != np.uint8:
            raise LtError("set_labels: expected a uint8 array, got %s" % a.dtype.name)
        if self._grid_shape is not None and a.shape != self._grid_shape:
            raise LtError("set_labels: expected shape (nz, ny, nx) = %s, got %s" % (self._grid_shape, a.shape))
        a = np.ascontiguousarray(a)
        if n_labels is None:
            used = a[a != LABEL_NONE]
            n_labels = int(used.max()) + 1 if used.size else 1
        self._ck(lib().lt_set_labels(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8)), a.size, int(n_labels)), "lt_set_labels")

    def labels_info(self):
        """The n_labels in force, 0 when no labels are set."""
        n = C.c_int()
        self._ck(lib().lt_labels_info(self._h, C.byref(n)), "lt_labels_info")
        return n.value

    def tally_label_sums(self, raw=False):
        """dict of arrays [n_labels] (one label without set_labels): weight (float64 sum of the label's voxels), voxels,
        filled (non-zero voxels; uint64), peak (float64: the largest voxel), peak_index (int64: the lowest flat index (z * ny
        + y) * nx + x that holds it; the first voxel of an all-zero label, -1 for a label without voxels) and, with raw=True
        (u64 fixed-point tally only), raw: the exact uint64 sums."""
        n = max(self.labels_info(), 1)
        out, rawbuf, rp = self._sum_buffers((n,), raw)
        vox, filled = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        peak, idx = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int64)
        self._ck(lib().lt_tally_label_sums(self._h, _dp(out), rp, vox.ctypes.data_as(_U64P), filled.ctypes.data_as(_U64P), _dp(peak),
                                           idx.ctypes.data_as(C.POINTER(C.c_int64))), "lt_tally_label_sums")
        res = dict(weight=out, voxels=vox, filled=filled, peak=peak, peak_index=idx)
        if raw:
            res["raw"] = rawbuf
        return res

    def tally_histogram(self, edges, raw=False):
        """(voxels uint64, weight) [n_labels, len(edges) + 1]: per label, class k = the voxels whose value (as weight) has k
        of the ascending ``edges`` at or below it, and the sum of their values.  raw=True (u64 fixed-point tally only): weight
        is the exact uint64 sums.  The cumulative histogram is voxels[:, ::-1].cumsum(1)[:, ::-1]."""
        e = _f64(edges).reshape(-1)
        n = max(self.labels_info(), 1)
        vox = np.zeros((n, e.size + 1), dtype=np.uint64)
        out, rawbuf, rp = self._sum_buffers((n, e.size + 1), raw)
        self._ck(lib().lt_tally_histogram(self._h, _dp(e), int(e.size), vox.ctypes.data_as(_U64P), _dp(out), rp), "lt_tally_histogram")
        return vox, (rawbuf if raw else out)

    # -- the tally along rays (lt.h: lt_tally_rays, lt_tally_view) ---------------------------------------------------------
    def _ray_buffers(self, shape, want, threshold):
        """(dict of output arrays of ``shape``, the five ctypes pointers in lt.h's order, threshold as a float)."""
        names = ray_wants(want)
        res, ptr = {}, []
        for key, group, dt in (("integral", "integral", np.float64), ("max", "max", np.float64), ("max_index", "max", np.int64),
                               ("first_t", "first", np.float64), ("first_index", "first", np.int64)):
            if group in names:
                res[key] = np.empty(shape, dtype=dt)
                ptr.append(res[key].ctypes.data_as(_DP if dt is np.float64 else _I64P))
            else:
                ptr.append(None)
        return res, ptr, 0.0 if threshold is None else float(threshold)

    def tally_rays(self, origins, dirs, t_range=None, threshold=None, want=RAY_WANTS):
        """The tally along rays o + t d (origins, dirs: float64 [n, 3]; t_range: [n, 2] = (t_lo, t_hi) per ray, one pair for all,
        or None = [0, inf)), walked voxel by voxel on the device.  A dict of arrays [n], by ``want``: "integral" -> integral (sum
        of voxel weight x length of the ray inside the voxel); "max" -> max (the largest voxel on the ray, as weight) and
        max_index (the flat index (z ny + y) nx + x of the first voxel along the ray that holds it, -1 for a ray that crosses no
        voxel); "first" -> first_index (the first voxel along the ray whose weight is >= ``threshold``) and first_t (the
        parameter at which the ray enters it; inf and -1 without one).  threshold=None is 0: the entry into the grid."""
        o, d = _f64(origins).reshape(-1, 3), _f64(dirs).reshape(-1, 3)
        n = o.shape[0]
        if d.shape[0] != n:
            raise LtError("tally_rays: %d origins and %d directions" % (n, d.shape[0]))
        tr = None if t_range is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t_range, dtype=np.float64), (n, 2)))
        res, p, thr = self._ray_buffers((n,), want, threshold)
        self._ck(lib().lt_tally_rays(self._h, _dp(o), _dp(d), _dp(tr), C.c_size_t(n), C.c_double(thr), *p), "lt_tally_rays")
        return res

    def tally_view(self, camera, f_distance, xs, ys, threshold=None, want=RAY_WANTS):
        """tally_rays along the rays of render_surface's pinhole camera (camera_rays), built on the device: a dict of arrays
        [len(ys), len(xs)], bit for bit what tally_rays returns for those rays."""
        cam = (C.c_double * 3)(*[float(x) for x in np.asarray(camera).ravel()[:3]])
        xs, ys = _f64(xs).reshape(-1), _f64(ys).reshape(-1)
        res, p, thr = self._ray_buffers((ys.size, xs.size), want, threshold)
        self._ck(lib().lt_tally_view(self._h, C.c_int(xs.size), C.c_int(ys.size), cam, C.c_double(float(f_distance)), _dp(xs), _dp(ys),
                                     C.c_double(thr), *p), "lt_tally_view")
        return res

    def read_counters(self):
        c = Counters()
        self._ck(lib().lt_read_counters(self._h, C.byref(c)), "lt_read_counters")
        return c.as_dict()

    def grid_device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(lib().lt_grid_device_ptr(self._h, C.byref(p), C.byref(n)), "lt_grid_device_ptr")
        return p.value, n.value

    def counters_device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(lib().lt_counters_device_ptr(self._h, C.byref(p), C.byref(n)), "lt_counters_device_ptr")
        return p.value, n.value

    def stream(self):
        return lib().lt_stream(self._h)

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, mhz, mem = C.c_int(), C.c_int(), C.c_size_t()
        self._ck(lib().lt_device_info(self._h, name, C.c_size_t(256), C.byref(cus), C.byref(mhz), C.byref(mem)),
                 "lt_device_info")
        return dict(name=name.value.decode(), cus=cus.value, clock_mhz=mhz.value, hbm_bytes=mem.value)

    # -- device-side queries ----------------------------------------------
    def intersect_rays(self, origins, dirs, tmax=None, use_bvh=True):
        o, d = _f64(origins).reshape(-1, 3), _f64(dirs).reshape(-1, 3)
        n = o.shape[0]
        tm = None if tmax is None else np.ascontiguousarray(np.broadcast_to(tmax, (n,)), dtype=np.float64)
        prim, t = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64)
        self._ck(lib().lt_intersect_rays(self._h, _dp(o), _dp(d), _dp(tm), C.c_size_t(n), C.c_int(int(use_bvh)),
                                         _ip(prim), _dp(t)), "lt_intersect_rays")
        return prim, t

    def triangle_intersect(self, origins, dirs, tris):
        o, d, t = _f64(origins).reshape(-1, 3), _f64(dirs).reshape(-1, 3), _f64(tris).reshape(-1, 9)
        out = np.empty(o.shape[0], dtype=np.float64)
        self._ck(lib().lt_triangle_intersect(self._h, _dp(o), _dp(d), _dp(t), C.c_size_t(o.shape[0]), _dp(out)),
                 "lt_triangle_intersect")
        return out

    def intersect_bounds(self, origins, dirs, boxes, tmax=None):
        o, d, b = _f64(origins).reshape(-1, 3), _f64(dirs).reshape(-1, 3), _f64(boxes).reshape(-1, 6)
        n = o.shape[0]
        tm = None if tmax is None else np.ascontiguousarray(np.broadcast_to(tmax, (n,)), dtype=np.float64)
        out = np.empty(n, dtype=np.int32)
        self._ck(lib().lt_intersect_bounds(self._h, _dp(o), _dp(d), _dp(tm), _dp(b), C.c_size_t(n), _ip(out)),
                 "lt_intersect_bounds")
        return out

    def eval(self, name, inp):
        fn = FN[name]
        k_in, k_out = _FN_SHAPE[fn]
        a = _f64(inp).reshape(-1, k_in)
        out = np.empty((a.shape[0], k_out), dtype=np.float64)
        self._ck(lib().lt_eval(self._h, C.c_int(fn), _dp(a), C.c_size_t(a.shape[0]), _dp(out)), "lt_eval")
        return out

    # -- light sub-path vertices (f4) ----------------------------------------
    def set_vertex_capture(self, max_vertices_per_photon):
        self._ck(lib().lt_set_vertex_capture(self._h, C.c_uint32(int(max_vertices_per_photon))), "lt_set_vertex_capture")
        self._max_vertices = int(max_vertices_per_photon)

    def read_vertices(self, n_photons):
        """-> (vertices [n_photons, K] record array of VERTEX_DTYPE, counts [n_photons] uint32) of the last launch."""
        k = getattr(self, "_captured_max_vertices", 0)     # the K in effect at the capturing launch
        v = np.zeros((int(n_photons), k), dtype=VERTEX_DTYPE)
        cnt = np.zeros(int(n_photons), dtype=np.uint32)
        self._ck(lib().lt_read_vertices(self._h, v.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p),
                                        C.c_uint64(int(n_photons))), "lt_read_vertices")
        return v, cnt

    # -- surface path tracing (f2) ------------------------------------------
    def set_surface_materials(self, mats):
        self._ck(lib().lt_set_surface_materials(self._h, mats, C.c_int(len(mats))), "lt_set_surface_materials")

    def set_lights(self, lights):
        self._ck(lib().lt_set_lights(self._h, lights, C.c_int(len(lights))), "lt_set_lights")

    def render_surface(self, camera, f_distance, xs, ys, rand_0, rand_1, light_choice, image, old=False):
        """rand_0 [H,W,S,D] and image [H,W,3] are updated in place (C-contiguous float64).  old=True: the recursive
        path_tracing_old integrator; light_choice is then [H,W,S,choices_per_sample] and image is overwritten."""
        H, W, S, D = rand_0.shape
        for a in (rand_0, rand_1, image):
            if a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"]:
                raise LtError("render_surface: tables and image must be C-contiguous float64")
        lc = np.ascontiguousarray(light_choice, dtype=np.int32)
        lc_ok = (lc.ndim == 4 and lc.shape[:3] == (H, W, S) and lc.shape[3] > 0) if old else lc.shape == rand_0.shape
        if rand_1.shape != rand_0.shape or not lc_ok or image.shape != (H, W, 3):
            raise LtError("render_surface: inconsistent table / image shapes")
        cam = (C.c_double * 3)(*[float(x) for x in np.asarray(camera).ravel()[:3]])
        xs, ys = _f64(xs), _f64(ys)
        if xs.size != W or ys.size != H:
            raise LtError("render_surface: xs / ys must have W / H entries")
        if old:
            self._ck(lib().lt_render_surface_old(self._h, C.c_int(W), C.c_int(H), C.c_int(S), C.c_int(D), cam,
                                                 C.c_double(f_distance), _dp(xs), _dp(ys), _dp(rand_0), _dp(rand_1),
                                                 _ip(lc), C.c_int(lc.shape[3]), _dp(image)), "lt_render_surface_old")
            return image
        self._ck(lib().lt_render_surface(self._h, C.c_int(W), C.c_int(H), C.c_int(S), C.c_int(D), cam,
                                         C.c_double(f_distance), _dp(xs), _dp(ys), _dp(rand_0), _dp(rand_1), _ip(lc),
                                         _dp(image)), "lt_render_surface")
        return image

    def rng_raw(self, seed, photon_id, count):
        out = np.empty(count, dtype=np.uint32)
        self._ck(lib().lt_rng_raw(self._h, C.c_uint64(seed), C.c_uint64(photon_id), C.c_uint32(count),
                                  out.ctypes.data_as(C.POINTER(C.c_uint32))), "lt_rng_raw")
        return out


_default_ctx = {}


def default_context(device_id=0):
    """Process-wide context per device, for the function-style API."""
    ctx = _default_ctx.get(device_id)
    if ctx is None:
        ctx = _default_ctx[device_id] = Context(device_id)
    return ctx
