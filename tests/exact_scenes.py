"""Scenes whose tally is an exact sum, and the limit grids of the deposit log.

With the right media every deposit is exactly representable and every sum of deposits is exact in any order, so the f64 and f32
grids, every counter and the conservation residual are the same BITS whichever route the deposits take (atomics, the log's
one-pass / two-pass / hot-tile partition, the spill of an exhausted log, one or several lanes).  Two families, every refractive
index 1 (media, n_above, n_below: no specular loss):

  unit    mu_s = 0: absorb = mu_a / mu_t = 1.0, a photon deposits exactly 1.0 at its first interaction and dies (steps ==
          photons).  Every voxel is an integer count: float sums are exact below 2^24 (f32) and 2^53 (f64).
  dyadic  mu_a == mu_s: absorb = 0.5, so a weight is 2^-k times a power of 10 from the roulette, a multiple of 2^-40 throughout:
          the f64 grid is the fixed-point grid times 2^-40 bit for bit, conservation_residual is 0.0 and w_absorbed is
          grid.sum().  (absorb = 1/4 grows powers of 3 and n = 1.4 loses a specular share: neither is exact.)

That a scene really has these properties is a fact about the ORACLE and is checked on the CPU, by tests/test_exact_scenes_cpu.py,
for every scene tests/test_gpu_exact_tally.py uses: a new scene goes into LIMIT_ARRANGEMENTS / ROUTE_SCENES / MESH_SCENES below and
`python -m pytest tests/test_exact_scenes_cpu.py -q -s` re-checks it (and prints photons, steps, tile coverage and the hottest
voxel) before any GPU run.  A plain helper module: no fixtures, no tests.
"""
import numpy as np

from oracle import oracle as O
from tests import scenes as S

TILE = (32, 32, 16)              # voxels of a deposit-log tile along x, y, z (kTileBX / BY / BZ of the library)
WIDE = 1.0e3                     # half width of a voxel on an axis that is one voxel thick: nothing is lost sideways
CLEAR = (0.0, 0.0, 0.0, 1.0)     # a non-interacting layer
ORACLE_THREADS = 16


def medium(kind, mu=1.0, g=0.0):
    """(mu_a, mu_s, g, n) of a unit or dyadic medium with mu_a = mu; mu = 0 is the clear medium."""
    assert kind in ("unit", "dyadic")
    if mu == 0.0:
        return CLEAR
    return (float(mu), 0.0, 0.0, 1.0) if kind == "unit" else (float(mu), float(mu), float(g), 1.0)


def pencil(pos=(0.0, 0.0, 0.0), direction=(0.0, 0.0, 1.0)):
    return dict(type=0, pos=tuple(pos), dir=tuple(direction), extra=(0.0,) * 6, start_medium=0)


def quad(corner, e1, e2, normal=(0.0, 0.0, 1.0), start_medium=0):
    """Cosine-lobe source on the parallelogram corner + s e1 + t e2."""
    return dict(type=1, pos=tuple(corner), dir=tuple(normal), extra=tuple(e1) + tuple(e2), start_medium=start_medium)


def face_quad(shape, origin, voxel, z=0.0):
    """The quad source that covers the grid's footprint in x and y at height z."""
    return quad((origin[0], origin[1], z), (shape[0] * voxel[0], 0.0, 0.0), (0.0, shape[1] * voxel[1], 0.0))


def _slab(kind, shape, origin, voxel, source, z_bounds, mus, g, max_steps):
    zb = [float(z) for z in z_bounds]
    assert len(zb) == len(mus) + 1
    media = [medium(kind, mu, g) for mu in mus]
    return S.Problem(media, tuple(int(n) for n in shape), tuple(float(x) for x in origin), tuple(float(x) for x in voxel),
                     layers=dict(z_bounds=zb, medium_idx=list(range(len(mus))), n_above=1.0, n_below=1.0),
                     source=source or pencil(), max_steps=max_steps)


def unit_slab(shape=(64, 64, 64), origin=(-3.2, -3.2, 0.0), voxel=(0.1, 0.1, 0.1), source=None, z_bounds=(0.0, np.inf),
              mus=(1.0,), max_steps=1000000):
    """A layered slab of unit media: layer k spans z_bounds[k] .. z_bounds[k + 1] with mu_a = mus[k] (0: a clear layer)."""
    return _slab("unit", shape, origin, voxel, source, z_bounds, mus, 0.0, max_steps)


def dyadic_slab(shape=(64, 64, 64), origin=(-3.2, -3.2, 0.0), voxel=(0.1, 0.1, 0.1), source=None, z_bounds=(0.0, np.inf),
                mus=(5.0,), g=0.9, max_steps=1000000):
    """A layered slab of dyadic media: mu_a = mu_s = mus[k] (0: a clear layer), anisotropy g in every layer."""
    return _slab("dyadic", shape, origin, voxel, source, z_bounds, mus, g, max_steps)


def _cornell(kind, n=64):
    """scenes.cornell(n) -- the mesh lives in LDS -- with only its media replaced: both of the family, n = 1."""
    prob = S.cornell(n)
    prob.media = [medium(kind, 0.1, 0.9), medium(kind, 1.0, 0.8)] if kind == "dyadic" else [medium(kind, 0.1), medium(kind, 1.0)]
    return prob


def dyadic_cornell(n=64):
    return _cornell("dyadic", n)


def unit_cornell(n=64):
    return _cornell("unit", n)


def thin_grid(ntx, nty, ntz, ragged=1, span=(6.0, 6.0, 6.0)):
    """(shape, origin, voxel) of the smallest grid with ntx x nty x ntz tiles: 32 (nt - 1) + r voxels along x and y, 16 (nt - 1) + r
    along z, r = `ragged` on every axis with more than one tile (on z when there is one tile in all) and 1 elsewhere -- the last
    tile of a long axis holds r voxels.  A long axis spans span[axis], centred on 0 in x and y and from 0 down in z; an axis
    that is one voxel thick spans +-WIDE."""
    nts = (int(ntx), int(nty), int(ntz))
    assert min(nts) >= 1 and 1 <= ragged <= min(TILE)
    long_ = [nt > 1 for nt in nts]
    if not any(long_):
        long_[2] = True
    shape = tuple(TILE[a] * (nts[a] - 1) + (ragged if long_[a] else 1) for a in range(3))
    origin, voxel = [], []
    for a in range(3):
        if shape[a] == 1:
            origin.append(-WIDE); voxel.append(2.0 * WIDE)
        else:
            origin.append(0.0 if a == 2 else -0.5 * span[a]); voxel.append(span[a] / shape[a])
    return shape, tuple(origin), tuple(voxel)


def n_tiles(shape):
    return int(np.prod([-(-int(shape[a]) // TILE[a]) for a in range(3)]))


def tile_histogram(grid):
    """Non-empty voxels per 32 x 32 x 16 tile of a grid [nz, ny, nx]: int64 [ntz, nty, ntx] (flat: the library's tile index
    (z nty + y) ntx + x)."""
    nz, ny, nx = grid.shape
    ntz, nty, ntx = -(-nz // TILE[2]), -(-ny // TILE[1]), -(-nx // TILE[0])
    full = np.zeros((ntz * TILE[2], nty * TILE[1], ntx * TILE[0]), dtype=bool)
    full[:nz, :ny, :nx] = grid != 0
    return full.reshape(ntz, TILE[2], nty, TILE[1], ntx, TILE[0]).sum(axis=(1, 3, 5), dtype=np.int64)


def assert_identical(got, want, what=""):
    """(grid, counters) twice: the grids' raw bytes are equal (same dtype and shape, -0.0 is not +0.0), `steps` and `photons`
    are equal and every w_* counter is equal with ==, not isclose."""
    g, c = got
    go, co = want
    assert g.dtype == go.dtype and g.shape == go.shape, "%s: %s %s against %s %s" % (what, g.dtype, g.shape, go.dtype, go.shape)
    bits = "u%d" % g.itemsize
    a, b = np.ascontiguousarray(g).reshape(-1).view(bits), np.ascontiguousarray(go).reshape(-1).view(bits)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        k = int(bad[0])
        raise AssertionError("%s: %d voxels differ; first at flat index %d (tile %s): %r against %r"
                             % (what, bad.size, k, _tile_of(k, g.shape), g.reshape(-1)[k], go.reshape(-1)[k]))
    assert set(c) == set(co), "%s: counter names differ" % what
    for k in ("photons", "steps"):
        assert int(c[k]) == int(co[k]), "%s: %s %d against %d" % (what, k, c[k], co[k])
    for k in sorted(c):
        if k.startswith("w_"):
            a, b = np.float64(c[k]), np.float64(co[k])
            assert a == b, "%s: %s %r against %r (difference %g)" % (what, k, float(a), float(b), float(a - b))


def _tile_of(flat, shape):
    nz, ny, nx = shape
    z, y, x = flat // (ny * nx), (flat // nx) % ny, flat % nx
    return (x // TILE[0], y // TILE[1], z // TILE[2])


# ---------------------------------------------------------------- the scenes of the GPU tests, by name
# Tile counts at which the deposit path changes form: 1024 | 1025 one pass | two passes, 4096 | 4097 the
# level-2 digit grows from 6 to 7 bits, 8192 | 8193 the hot-tile form ends, 65536 | 65537 the log ends (atomics).
LIMIT_COUNTS_Z = (1, 2, 1024, 1025, 4096, 4097, 8192, 8193, 65536, 65537)
LIMIT_COUNTS_ROW = (1025, 8193, 65536, 65537)
RAGGED = 5          # voxels of the last tile along a long axis
RAGGED_CORNER = 8   # the same where the last tile is ragged along two or three axes and lies in the far corner


def limit_arrangements():
    """name -> (ntx, nty, ntz) of every limit grid."""
    arr = {"z%d" % n: (1, 1, n) for n in LIMIT_COUNTS_Z}
    arr.update({"x%d" % n: (n, 1, 1) for n in LIMIT_COUNTS_ROW})
    arr.update({"y%d" % n: (1, n, 1) for n in LIMIT_COUNTS_ROW})
    arr["xz128"] = (128, 1, 128)
    arr["xyz8x8x16"] = (8, 8, 16)
    return arr


LIMIT_ARRANGEMENTS = limit_arrangements()


def limit_scene(kind, name):
    """(Problem, photons) of the limit grid `name` (LIMIT_ARRANGEMENTS) in the `kind` family.

    z columns: a pencil beam down the column, which is 2 (unit) or 4 (dyadic) mean free paths deep.  Rows, the sheet and the
    block: a cosine quad source over the whole top face, so that every tile is fed -- a unit photon deposits once, on its first
    flight, and a pencil beam would leave all of them in one column; 1.5 (unit) / 3 (dyadic) mean free paths deep where z is long.
    Photon counts: a unit photon costs one step, a dyadic one about twenty."""
    nts = LIMIT_ARRANGEMENTS[name]
    tiles = nts[0] * nts[1] * nts[2]
    column = nts[0] == 1 and nts[1] == 1
    corner = nts[2] > 1 and not column       # the last tile is a corner at the far end: r x r voxels that few photons reach
    ragged = RAGGED_CORNER if corner else RAGGED
    if kind == "unit":
        depth = 2.0 if column else 1.0
        shape, origin, voxel = thin_grid(*nts, ragged=ragged, span=(6.0, 6.0, depth))
        src = pencil() if column else face_quad(shape, origin, voxel)
        n = 4000000 if corner else int(min(4000000, max(100000, 60 * tiles)))
        return unit_slab(shape, origin, voxel, src, mus=(1.0,)), n
    depth = 4.0 if column or corner else 3.0
    shape, origin, voxel = thin_grid(*nts, ragged=ragged, span=(6.0, 6.0, depth))
    src = pencil() if column else face_quad(shape, origin, voxel)
    n = 400000 if corner else int(min(200000, max(50000, 3 * tiles)))
    return dyadic_slab(shape, origin, voxel, src, mus=(0.5,), g=0.9), n


def route_scene(name):
    """(kind, Problem) of the 3-D scenes the routes are compared on: (100, 70, 33) is no multiple of the tile in any axis, 128^3
    is 128 whole tiles; a dyadic slab, a dyadic three-layer slab with a clear gap, a unit slab under a quad source."""
    grids = {"odd": ((100, 70, 33), (-5.0, -3.5, 0.0), (0.1,) * 3), "128": ((128,) * 3, (-6.4, -6.4, 0.0), (0.1,) * 3)}
    what, gname = name.split("-")
    shape, origin, voxel = grids[gname]
    if what == "dyadic":
        return "dyadic", dyadic_slab(shape, origin, voxel, mus=(1.0,), g=0.9)
    if what == "gap":
        return "dyadic", dyadic_slab(shape, origin, voxel, z_bounds=(0.0, 0.4, 0.9, np.inf), mus=(2.0, 0.0, 1.0), g=0.8)
    assert what == "unit"
    ex, ey = 0.6 * shape[0] * voxel[0], 0.6 * shape[1] * voxel[1]
    return "unit", unit_slab(shape, origin, voxel, quad((-0.5 * ex, -0.5 * ey, 0.0), (ex, 0.0, 0.0), (0.0, ey, 0.0)), mus=(1.0,))


ROUTE_SCENES = tuple("%s-%s" % (w, g) for g in ("odd", "128") for w in ("dyadic", "gap", "unit"))
ROUTE_PHOTONS = 200000
MESH_SCENES = {"dyadic_cornell": ("dyadic", dyadic_cornell, 60000), "unit_cornell": ("unit", unit_cornell, 200000)}
SEED = 23



def shards(n):
    """Three ragged (photon_offset, count) shards of a launch of n photons."""
    a, b = (n * 17) // 100 + 3, n // 2 + 1
    return ((0, a), (a, b), (a + b, n - a - b))


_oracle_cache = {}


def oracle_run(key, prob, n, seed=SEED, photon_offset=0):
    """(f64 grid, u64 grid, counters) of the f64 oracle walk, computed once per key and shared by the tests that follow one
    another (the last few results are kept: the largest pair of grids is 200 MB): never modify the arrays."""
    k = (key, n, seed, photon_offset)
    if k not in _oracle_cache:
        while len(_oracle_cache) >= 6:
            _oracle_cache.pop(next(iter(_oracle_cache)))
        g, fx, c = prob.oracle().run(n, seed=seed, photon_offset=photon_offset, threads=ORACLE_THREADS, want_fx=True)
        g.setflags(write=False); fx.setflags(write=False)
        _oracle_cache[k] = (g, fx, c)
    return _oracle_cache[k]


def oracle_as(dtype, result):
    """The oracle's result in a tally's raw type: (grid, counters) as read_grid_raw / read_counters give them."""
    g, fx, c = result
    if dtype == "u64fx":
        return fx, c
    if dtype == "f64":
        return g, c
    assert dtype == "f32"
    g32 = g.astype(np.float32)
    assert np.array_equal(g32.astype(np.float64), g), "the scene's voxels are not exact in f32"
    return g32, c


def check_exact(kind, result, limit=False, one_step=True):
    """The conditions that make a scene exact (module docstring), on an oracle result; `limit`: those of a limit scene too;
    one_step=False: a unit photon may take more steps than one (a mesh walk counts the surfaces it crosses).
    Returns dict(steps, coverage, first, last, hottest) for the report."""
    g, fx, c = result
    assert g.tobytes() == (fx.astype(np.float64) * 2.0 ** -40).tobytes(), "the f64 grid is not the fixed-point grid x 2^-40"
    assert O.conservation_residual(c) == 0.0, O.conservation_residual(c)
    assert c["w_absorbed"] == g.sum(), (c["w_absorbed"], g.sum())
    assert c["w_absorbed"] > 0
    if kind == "unit":
        assert np.array_equal(g, np.round(g)) and g.max() < 2 ** 24
        assert c["steps"] == c["photons"] if one_step else c["steps"] >= c["photons"]
    hist = tile_histogram(g).reshape(-1)
    cover = float((hist > 0).mean())
    if limit:
        assert cover >= 0.75, "only %.1f %% of the tiles hold anything" % (100 * cover)
        assert hist[0] > 0 and hist[-1] > 0, "first / last tile: %d / %d non-empty voxels" % (hist[0], hist[-1])
        assert float(g.max()) * 2.0 ** 40 < 2.0 ** 63
    return dict(steps=int(c["steps"]), coverage=cover, first=int(hist[0]), last=int(hist[-1]), hottest=float(g.max()))
