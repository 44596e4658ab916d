"""Transport problems used by the tests, described ONCE and applied both to the
CPU oracle (oracle.OracleScene) and to the HIP path (Context.set_*), so both sides
see identical inputs.  C1..C4 follow BASELINE.json's configs / SURVEY.md 8(d)."""
import numpy as np

from light_transport_amd.src import bvh_new as B
from light_transport_amd.src import constants as K
from light_transport_amd.src import cornell_box as cb
from oracle import oracle as O


class Problem:
    def __init__(self, media, grid_shape, origin, voxel, layers=None, mesh=None, source=None, max_steps=1000000):
        self.media, self.grid_shape, self.origin, self.voxel = media, grid_shape, origin, voxel
        self.layers, self.mesh, self.max_steps = layers, mesh, max_steps
        self.source = source or dict(type=0, pos=(0.0, 0.0, 0.0), dir=(0.0, 0.0, 1.0), extra=(0.0,) * 6, start_medium=0)

    def oracle(self):
        return O.OracleScene(self.media, self.grid_shape, self.origin, self.voxel, layers=self.layers, mesh=self.mesh,
                             source=self.source, max_steps=self.max_steps)

    def apply(self, ctx, dtype="f64"):
        ctx.set_media(self.media)
        if self.layers is not None:
            ctx.set_layers(self.layers["z_bounds"], self.layers["medium_idx"], self.layers.get("n_above", 1.0),
                           self.layers.get("n_below", 1.0))
        else:
            ctx.set_mesh(self.mesh["verts"], self.mesh["med_front"], self.mesh["med_back"], self.mesh["nodes"])
        ctx.set_grid(self.grid_shape, self.origin, self.voxel, dtype)
        s = self.source
        ctx.set_source(s.get("type", 0), s["pos"], s["dir"], s.get("extra"), s.get("start_medium", 0))
        ctx.set_max_steps(self.max_steps)
        ctx.set_tally_quantity("absorbed")
        return ctx


def slab(n=64, voxel=0.4, media=((0.1, 10.0, 0.9, 1.0),), thickness=np.inf, n_above=1.0, n_below=1.0, **kw):
    """C1 (n=64, voxel 0.4) / C2 (n=256, voxel 0.1): homogeneous semi-infinite slab, pencil beam."""
    half = n * voxel / 2
    return Problem(list(media), (n, n, n), (-half, -half, 0.0), (voxel,) * 3,
                   layers=dict(z_bounds=[0.0, thickness], medium_idx=[0], n_above=n_above, n_below=n_below), **kw)


def two_layer(n=64, voxel=0.2, **kw):
    """C3: epidermis 0-0.1 mm over dermis, ambient n = 1 (values of SURVEY.md 8(d))."""
    half = n * voxel / 2
    media = [(0.43, 10.7, 0.79, 1.5), (0.27, 18.7, 0.82, 1.4)]
    return Problem(media, (n, n, n), (-half, -half, 0.0), (voxel,) * 3,
                   layers=dict(z_bounds=[0.0, 0.1, np.inf], medium_idx=[0, 1], n_above=1.0, n_below=1.0), **kw)


def cornell_scene(split_method=1):
    """The 30-triangle Cornell cavity + cone of config 4, in BVH order, with media labels."""
    dim = 7.5
    walls = (cb.get_cornell_box(dim, K.GLASS_MAT, K.GLASS_MAT, K.GLASS_MAT) + cb.get_front_wall(dim, K.GLASS_MAT)
             + cb.get_light_quad(dim, K.GLASS_MAT))
    cone = cb.get_cone(K.GLASS_MAT)
    for t in walls:   # normals point into the cavity: front = cavity medium, back = exterior
        t.med_front, t.med_back = 0, -1
    for t in cone:    # normals point out of the cone: front = cavity medium, back = cone medium
        t.med_front, t.med_back = 0, 1
    ordered, linear = B.build_linear_bvh(walls + cone, split_method)
    return ordered, linear


def cornell(n=64, **kw):
    """C4: C1's medium fills the cube, a cone of a second medium sits in it, cosine source on the ceiling quad."""
    dim = 7.5
    ordered, linear = cornell_scene()
    mesh = dict(verts=B.triangles_array(ordered), med_front=np.array([t.med_front for t in ordered], np.int32),
                med_back=np.array([t.med_back for t in ordered], np.int32), nodes=B.linear_bvh_arrays(linear))
    media = [(0.1, 10.0, 0.9, 1.0), (1.0, 5.0, 0.8, 1.5)]
    src = dict(type=1, pos=(-1.0, dim, -1.0), dir=(0.0, -1.0, 0.0), extra=(2.0, 0.0, 0.0, 0.0, 0.0, 2.0), start_medium=0)
    voxel = 2 * dim / n
    return Problem(media, (n, n, n), (-dim, -dim, -dim), (voxel,) * 3, mesh=mesh, source=src, **kw)


def transformed(prob, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """The same problem in other units and another frame: a new Problem in which every length x is x * scale + shift (grid
    origin, z_bounds -- inf stays inf --, source position, mesh vertices, BVH bounds), every extent (voxel, the source's edge
    vectors) is multiplied by scale and mu_a, mu_s are divided by it; g, n, directions, grid shape, max_steps and the medium
    ids stay.  With scale a power of two and no shift every value is scaled exactly."""
    scale = float(scale)
    assert scale > 0
    sh = np.asarray(shift, dtype=np.float64)

    def move(x):
        return np.asarray(x, dtype=np.float64) * scale + sh

    media = [(m[0] / scale, m[1] / scale, m[2], m[3]) for m in prob.media]
    layers = mesh = None
    if prob.layers is not None:
        layers = dict(prob.layers)
        layers["z_bounds"] = [float(z) * scale + sh[2] for z in prob.layers["z_bounds"]]
        layers["medium_idx"] = list(prob.layers["medium_idx"])
    if prob.mesh is not None:
        nodes = {k: np.array(v) for k, v in prob.mesh["nodes"].items()}
        nodes["lo"], nodes["hi"] = move(nodes["lo"]), move(nodes["hi"])
        mesh = dict(verts=move(prob.mesh["verts"]), med_front=prob.mesh["med_front"].copy(), med_back=prob.mesh["med_back"].copy(),
                    nodes=nodes)
        # every bound is a vertex coordinate: it went through the same rounding as the vertex
        v = mesh["verts"].reshape(-1, 3)
        assert np.array_equal(nodes["lo"][0], v.min(axis=0)) and np.array_equal(nodes["hi"][0], v.max(axis=0))
    s = prob.source
    src = dict(s, pos=tuple(float(x) for x in move(s["pos"])), dir=tuple(s["dir"]),
               extra=tuple(float(x) * scale for x in s.get("extra", (0.0,) * 6)))
    return Problem(media, tuple(prob.grid_shape), tuple(float(x) for x in move(prob.origin)),
                   tuple(float(x) * scale for x in prob.voxel), layers=layers, mesh=mesh, source=src, max_steps=prob.max_steps)


def assert_grid_close(g, go, rtol=1e-9, atol=1e-12, max_bad=0):
    d = np.abs(g - go)
    bad = int((d > atol + rtol * np.abs(go)).sum())
    assert bad <= max_bad, "%d voxels outside |d| <= %g + %g*E (max abs %g)" % (bad, atol, rtol, d.max())


def icosphere(subdiv=3, radius=1.0, center=(0.0, 0.0, 0.0)):
    """(vertices, faces) of a subdivided icosahedron, outward-facing: 20 * 4^subdiv triangles."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + np.asarray(center, dtype=np.float64), np.array(f, dtype=np.int64)


def sphere_in_box(subdiv=4, n=48, split_method=0, balls=((1.5, (0.3, -0.2, 0.1)),), **kw):
    """f1 scene: a finely tessellated sphere (20 * 4^subdiv triangles; 5120 at subdiv 4 -- beyond the LDS
    budget, so the walk traverses it in global memory) of an absorbing medium inside a closed box.
    balls: (radius, centre) of every sphere -- several disjoint ones give triangle counts between the powers of four."""
    from light_transport_amd.src.io import triangles_from_mesh
    dim = 4.0
    walls = cb.get_cornell_box(dim, K.GLASS_MAT, K.GLASS_MAT, K.GLASS_MAT) + cb.get_front_wall(dim, K.GLASS_MAT) \
        + cb.get_light_quad(dim, K.GLASS_MAT)
    for t in walls:
        t.med_front, t.med_back = 0, -1
    ball = []
    for radius, centre in balls:
        vs, fs = icosphere(subdiv, radius, centre)
        ball += triangles_from_mesh(vs, fs, K.GLASS_MAT)
    for t in ball:
        t.med_front, t.med_back = 0, 1
    ordered, linear = B.build_linear_bvh(walls + ball, split_method)
    mesh = dict(verts=B.triangles_array(ordered), med_front=np.array([t.med_front for t in ordered], np.int32),
                med_back=np.array([t.med_back for t in ordered], np.int32), nodes=B.linear_bvh_arrays(linear))
    media = [(0.05, 5.0, 0.8, 1.0), (0.8, 8.0, 0.9, 1.37)]
    src = dict(type=1, pos=(-1.0, dim, -1.0), dir=(0.0, -1.0, 0.0), extra=(2.0, 0.0, 0.0, 0.0, 0.0, 2.0), start_medium=0)
    voxel = 2 * dim / n
    return Problem(media, (n, n, n), (-dim, -dim, -dim), (voxel,) * 3, mesh=mesh, source=src, **kw), ordered, linear


def open_sheets(n=24, **kw):
    """An OPEN mesh beyond the LDS budget: a bumpy 40 x 40 sheet (3200 triangles) over an exactly flat 30 x 30 one (1800), no box
    around them -- photons roam all around the mesh, outside its bounding box too, and the flat sheet has zero extent on z.
    Medium 1 between the sheets, exterior below the flat one; a handful of zero-area triangles are mixed in."""
    from light_transport_amd.src.io import triangles_from_mesh

    def sheet(m, half, zf):
        xs = np.linspace(-half, half, m + 1)
        X, Y = np.meshgrid(xs, xs, indexing="ij")
        V = np.stack([X, Y, zf(X, Y)], axis=-1).reshape(-1, 3)
        idx = lambda i, j: i * (m + 1) + j      # noqa: E731
        F = []
        for i in range(m):
            for j in range(m):      # counter-clockwise seen from +z: normals point up
                F += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
        return V, np.array(F)
    v1, f1 = sheet(40, 4.0, lambda X, Y: 0.3 * np.sin(1.3 * X) * np.cos(0.9 * Y))
    v2, f2 = sheet(30, 3.0, lambda X, Y: np.full_like(X, -2.0))
    bumpy = triangles_from_mesh(v1, f1, K.GLASS_MAT, drop_degenerate=False)
    flat = triangles_from_mesh(v2, f2, K.GLASS_MAT, drop_degenerate=False)
    deg = triangles_from_mesh(np.array([[0.5, 0.5, 1.0], [1.5, 1.5, 1.0], [1.0, 1.0, 1.0], [2.0, 0.0, -1.0]]),
                              np.array([(0, 1, 2), (3, 3, 3), (0, 0, 1)]), K.GLASS_MAT, drop_degenerate=False)      # collinear / coincident vertices
    for t in bumpy + deg:
        t.med_front, t.med_back = 0, 1
    for t in flat:
        t.med_front, t.med_back = 1, -1
    ordered, linear = B.build_linear_bvh(bumpy + flat + deg, 0)
    mesh = dict(verts=B.triangles_array(ordered), med_front=np.array([t.med_front for t in ordered], np.int32),
                med_back=np.array([t.med_back for t in ordered], np.int32), nodes=B.linear_bvh_arrays(linear))
    media = [(0.05, 5.0, 0.8, 1.0), (0.8, 8.0, 0.9, 1.37)]
    src = dict(type=0, pos=(0.1, -0.2, 3.0), dir=(0.05, 0.02, -1.0), extra=(0.0,) * 6, start_medium=0)
    return Problem(media, (n, n, n), (-6.0, -6.0, -6.0), (12.0 / n,) * 3, mesh=mesh, source=src, **kw), ordered, linear


def slab_as_mesh(media, z_bounds, medium_idx=None, n_above=1.0, n_below=1.0, direction=(0.0, 0.0, 1.0),
                 entry=(0.003, -0.002), half_width=10.0, cells=1, closed=True, dz=0.01, columns=8, grid_above=0.0,
                 split_method=0, **kw):
    """One layered slab described both ways: as z_bounds for the layered walk and as a closed triangle mesh for the mesh
    walks, which must then give the same reflectance, transmittance and depth profile.

    The mesh: a lid 0.1 above the first plane, the slab's planes, a floor 0.2 below the last; per slice four side walls at
    |x| = |y| = half_width.  Every plane is `cells` x `cells` quads of two triangles, counter-clockwise seen from +z
    (normal +z: med_front, the side the normal points to, is the DEEPER slice); wall triangles face inwards (front = the
    slice's medium, back = -1).  Two media are appended to `media`: `amb` = (0, 0, 0, n_above), non-interacting, between lid
    and slab, and `det` = (400, 0, 0, n_below), a pure absorber below the slab that takes every transmitted photon at its
    first interaction (e^-80 of them reach the floor) -- so T is the weight absorbed in the detector rows, R (specular +
    diffuse) is w_escaped_mesh (the lid's far side is the index-matched exterior) and A(z) the slab rows.  The pencil beam
    starts in `amb` (start_medium != 0), 0.05 above the first plane, aimed at `entry` on it; the layered beam starts AT
    `entry`.  Keep `entry` off the quads' edges and diagonals (x = y modulo the cell): the f32 triangle test is not
    watertight on a shared edge.
    closed=False leaves lid, floor and walls out: a photon in `amb` with nothing ahead leaves through the walk's
    "non-interacting and nothing ahead" exit, and the detector slice is bounded by its plane alone.

    The grid, shared by both problems: `columns` x `columns` columns over |x|, |y| <= half_width plus one guard column on
    every side (weight there lies outside the mesh's walls), rows of dz from `grid_above` above the first plane to the floor.
    Returns (mesh problem, layered problem, slab rows, detector rows) -- the rows as slices of the z axis."""
    from light_transport_amd.src.io import triangles_from_mesh
    zb = [float(z) for z in z_bounds]
    assert np.all(np.isfinite(zb)) and len(zb) >= 2
    nl = len(zb) - 1
    medium_idx = list(range(nl)) if medium_idx is None else [int(m) for m in medium_idx]
    amb, det = len(media), len(media) + 1
    all_media = [tuple(m) for m in media] + [(0.0, 0.0, 0.0, float(n_above)), (400.0, 0.0, 0.0, float(n_below))]
    L = float(half_width)
    planes = [zb[0] - 0.1] + zb + [zb[-1] + 0.2]                  # lid, the slab's planes, floor
    slices = [amb] + medium_idx + [det]                           # the medium between planes[k] and planes[k + 1]
    xs = np.linspace(-L, L, cells + 1)
    verts, faces, front, back = [], [], [], []

    def quad(p00, p10, p11, p01, toward, mf, mb):
        """Two triangles over the quad, wound so that the normal points along `toward`."""
        tris = [(p00, p10, p11), (p00, p11, p01)]
        if np.dot(np.cross(np.subtract(p10, p00), np.subtract(p11, p00)), toward) < 0:
            tris = [(a, c, b) for a, b, c in tris]
        for t in tris:
            faces.append((len(verts), len(verts) + 1, len(verts) + 2))
            verts.extend(t)
            front.append(mf); back.append(mb)

    for k, z in enumerate(planes):
        if not closed and k in (0, len(planes) - 1):
            continue
        mb = slices[k - 1] if k > 0 else -1
        mf = slices[k] if k < len(slices) else -1
        for i in range(cells):
            for j in range(cells):
                quad((xs[i], xs[j], z), (xs[i + 1], xs[j], z), (xs[i + 1], xs[j + 1], z), (xs[i], xs[j + 1], z), (0, 0, 1), mf, mb)
    if closed:
        for k, m in enumerate(slices):
            za, zc = planes[k], planes[k + 1]
            for i in range(cells):
                a, b = xs[i], xs[i + 1]
                quad((L, a, za), (L, b, za), (L, b, zc), (L, a, zc), (-1, 0, 0), m, -1)
                quad((-L, a, za), (-L, b, za), (-L, b, zc), (-L, a, zc), (1, 0, 0), m, -1)
                quad((a, L, za), (b, L, za), (b, L, zc), (a, L, zc), (0, -1, 0), m, -1)
                quad((a, -L, za), (b, -L, za), (b, -L, zc), (a, -L, zc), (0, 1, 0), m, -1)
    tris = triangles_from_mesh(np.array(verts, dtype=np.float64), np.array(faces), K.GLASS_MAT, drop_degenerate=False)
    for t, mf, mb in zip(tris, front, back):
        t.med_front, t.med_back = mf, mb
    ordered, linear = B.build_linear_bvh(tris, split_method)
    mesh = dict(verts=B.triangles_array(ordered), med_front=np.array([t.med_front for t in ordered], np.int32),
                med_back=np.array([t.med_back for t in ordered], np.int32), nodes=B.linear_bvh_arrays(linear))

    d = np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    assert d[2] > 0
    e = np.array([entry[0], entry[1], zb[0]])
    start = e - d * (0.05 / d[2])
    above, n_slab, n_det = int(round(grid_above / dz)), int(round((zb[-1] - zb[0]) / dz)), int(round(0.2 / dz))
    w = 2 * L / columns
    shape, origin, voxel = (columns + 2, columns + 2, above + n_slab + n_det), (-L - w, -L - w, zb[0] - above * dz), (w, w, dz)
    mesh_prob = Problem(all_media, shape, origin, voxel, mesh=mesh,
                        source=dict(type=0, pos=tuple(start), dir=tuple(d), extra=(0.0,) * 6, start_medium=amb), **kw)
    layered_prob = Problem([tuple(m) for m in media], shape, origin, voxel,
                           layers=dict(z_bounds=zb, medium_idx=medium_idx, n_above=float(n_above), n_below=float(n_below)),
                           source=dict(type=0, pos=tuple(e), dir=tuple(d), extra=(0.0,) * 6, start_medium=0), **kw)
    return mesh_prob, layered_prob, slice(above, above + n_slab), slice(above + n_slab, above + n_slab + n_det)


ANCHOR_SCENES = dict(       # slab_as_mesh arguments of the scenes that anchor the mesh walks to the layered walk
    two_layer=dict(media=[(0.43, 10.7, 0.79, 1.5), (0.27, 18.7, 0.82, 1.4)], z_bounds=[0.0, 0.1, 0.5]),      # skin, in air
    two_layer_tilted=dict(media=[(0.43, 10.7, 0.79, 1.5), (0.27, 18.7, 0.82, 1.4)], z_bounds=[0.0, 0.1, 0.5],
                          direction=(0.5, 0.3, 1.0), n_below=1.33),
    # Wang-Jacques-Zheng 1995, Table 3: three mismatched layers (n = 1.37 in air)
    table3=dict(media=[(1.0, 100.0, 0.9, 1.37), (1.0, 10.0, 0.0, 1.37), (2.0, 10.0, 0.7, 1.37)], z_bounds=[0.0, 0.1, 0.2, 0.4]),
    # the same paper's Table 1 (van de Hulst): matched 0.02 cm slab
    van_de_hulst=dict(media=[(10.0, 90.0, 0.75, 1.0)], z_bounds=[0.0, 0.02], half_width=2.0, dz=0.001),
)
_anchor_cache = {}


def anchor_scene(name, **kw):
    """slab_as_mesh(**ANCHOR_SCENES[name], **kw), built once per argument set and shared (never modified) by the tests."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _anchor_cache:
        _anchor_cache[key] = slab_as_mesh(**dict(ANCHOR_SCENES[name], **kw))
    return _anchor_cache[key]


def chain_mesh(T, seed=5):
    """T small triangles strung along x under a flattened tree that is a CHAIN: every interior node splits one triangle off
    (pre-order: interior i at 2i, its leaf at 2i + 1, the rest behind it) -- depth T - 1.  Returns (verts [T, 3, 3], nodes)."""
    rs = np.random.RandomState(seed)
    verts = np.zeros((T, 3, 3))
    for k in range(T):
        verts[k] = np.array([0.3 * k, 0.0, 0.0]) + rs.uniform(-0.12, 0.12, size=(3, 3))
    lo, hi = verts.min(axis=1), verts.max(axis=1)
    N = 2 * T - 1
    nodes = dict(lo=np.zeros((N, 3)), hi=np.zeros((N, 3)), offset=np.zeros(N, np.int32), n_prims=np.zeros(N, np.int32),
                 axis=np.zeros(N, np.int32))
    for i in range(T - 1):
        nodes["lo"][2 * i], nodes["hi"][2 * i] = lo[i:].min(axis=0), hi[i:].max(axis=0)
        nodes["offset"][2 * i] = 2 * i + 2                                  # second child
        nodes["lo"][2 * i + 1], nodes["hi"][2 * i + 1] = lo[i], hi[i]
        nodes["offset"][2 * i + 1], nodes["n_prims"][2 * i + 1] = i, 1
    nodes["lo"][N - 1], nodes["hi"][N - 1] = lo[T - 1], hi[T - 1]
    nodes["offset"][N - 1], nodes["n_prims"][N - 1] = T - 1, 1
    return verts, nodes


def chain_rays(verts, n, seed=6):
    """Rays aimed at (or just past) random points of random triangles of a chain_mesh, from origins around the chain: most
    hit, many cross the boxes of several links, a quarter run nearly along the chain's axis (every level is entered)."""
    rs = np.random.RandomState(seed)
    T = len(verts)
    o = rs.uniform(-1, 0.3 * T + 1, size=(n, 3)) * [1, 0, 0] + rs.uniform(-1, 1, size=(n, 3)) * [0, 1, 1]
    o[: n // 4, 1:] *= 0.05
    k = rs.randint(0, T, n)
    bary = rs.dirichlet([1, 1, 1], n)
    tgt = np.einsum("nk,nkc->nc", bary, verts[k]) + rs.normal(0, 0.03, size=(n, 3))
    d = tgt - o
    return o, d / np.linalg.norm(d, axis=1, keepdims=True), k


def g8_inputs(g8, name):
    """Build the mesh (my BVH builder over the fixture's triangles) and tables of a G8 render."""
    from light_transport_amd.src.io import triangles_from_mesh
    verts = g8[name + "_verts"]
    tris = triangles_from_mesh(verts.reshape(-1, 3), np.arange(len(verts) * 3).reshape(-1, 3), K.GLASS_MAT,
                               drop_degenerate=False)
    for k, t in enumerate(tris):
        t.fixture_index = k
    ordered, linear = B.build_linear_bvh(tris)
    order = np.array([t.fixture_index for t in ordered])
    mesh = dict(verts=B.triangles_array(ordered), med_front=-np.ones(len(ordered), np.int32),
                med_back=-np.ones(len(ordered), np.int32), nodes=B.linear_bvh_arrays(linear))
    H, W, S, D = g8[name + "_rand_0"].shape
    return dict(mesh=mesh, mats=g8[name + "_mats"][order], lights=g8[name + "_lights"], camera=g8["camera"],
                f_distance=float(g8["f_distance"]), xs=np.linspace(-1, 1, W),
                ys=np.linspace(1 / (W / H), -1 / (W / H), H),   # Scene.top / bottom, scene.py:60-63
                rand_0=g8[name + "_rand_0"], rand_1=g8[name + "_rand_1"], light_choice=g8[name + "_light_choice"],
                shape=(H, W, S, D))


def check_g8_image(img, rand_0_after, g8, name):
    """Exact-arithmetic parity target: the reference render with a correct nearest hit ('brute').  Against the
    reference as shipped ('asis') only the few pixels reached through its BVH bug B3 may differ."""
    ref = g8[name + "_brute_image"]
    np.testing.assert_allclose(img, ref, rtol=1e-9, atol=1e-12)
    marks = np.isinf(g8[name + "_brute_rand_0_after"])
    assert np.array_equal(np.isinf(rand_0_after), marks) and marks.sum() > 100
    asis = g8[name + "_asis_image"]
    bad = int((np.abs(img - asis).max(axis=2) > 1e-9).sum())
    assert bad <= 8, "%d pixels differ from the reference-as-shipped render" % bad
    assert img.sum() > 10 and (img.max(axis=2) > 0.2).sum() > 50


def check_g9_image(img, rand_0_after, g9, name):
    """path_tracing_old.render_scene as the reference ran it (correct nearest hit), incl. the markers in rand_0."""
    np.testing.assert_allclose(img, g9[name + "_image"], rtol=1e-9, atol=1e-12)
    marks = np.isinf(g9[name + "_rand_0_after"])
    assert np.array_equal(np.isinf(rand_0_after), marks) and marks.sum() > 100
    assert g9[name + "_shadow_rays"].max() > 4 and img.sum() > 10   # the recursion really branched


def obj_in_box(verts, faces, n=40, split_method=0, half=4.0, **kw):
    """f3 scene: a mesh that came through the OBJ loader (G10: teapot / cow / pumpkin of the reference's assets),
    scaled to fit and centred in a closed box, SAH-built; an absorbing medium on the back side of its triangles.
    Returns (problem, ordered triangles, linear BVH, index of every ordered mesh triangle in `faces` or -1 for walls)."""
    from light_transport_amd.src.io import triangles_from_mesh
    v = np.asarray(verts, dtype=np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    scale = 0.6 * 2 * half / float((hi - lo).max())
    shift = -0.5 * (lo + hi) * scale
    walls = cb.get_cornell_box(half, K.GLASS_MAT, K.GLASS_MAT, K.GLASS_MAT) + cb.get_front_wall(half, K.GLASS_MAT) \
        + cb.get_light_quad(half, K.GLASS_MAT)
    for t in walls:
        t.med_front, t.med_back, t.face_index = 0, -1, -1
    body = triangles_from_mesh(v, faces, K.GLASS_MAT, scale, shift, drop_degenerate=False)
    for k, t in enumerate(body):
        t.med_front, t.med_back, t.face_index = 0, 1, k
    ordered, linear = B.build_linear_bvh(walls + body, split_method)
    mesh = dict(verts=B.triangles_array(ordered), med_front=np.array([t.med_front for t in ordered], np.int32),
                med_back=np.array([t.med_back for t in ordered], np.int32), nodes=B.linear_bvh_arrays(linear))
    media = [(0.05, 5.0, 0.8, 1.0), (0.8, 8.0, 0.9, 1.37)]
    src = dict(type=1, pos=(-1.0, half, -1.0), dir=(0.0, -1.0, 0.0), extra=(2.0, 0.0, 0.0, 0.0, 0.0, 2.0), start_medium=0)
    voxel = 2 * half / n
    prob = Problem(media, (n, n, n), (-half, -half, -half), (voxel,) * 3, mesh=mesh, source=src, **kw)
    return prob, ordered, linear, np.array([t.face_index for t in ordered]), scale, shift


def write_obj(path, verts, faces, degenerate_every=0):
    """A triangle mesh as OBJ text that exercises every form src/io.read_obj accepts; reading it back must give verts
    and faces (plus the zero-area triangles injected below).  Written: comment / mtllib / o lines before the data,
    vn / vt / s / g / usemtl lines between the vertices and the faces and `usemtl` again every 500 face lines; `v` lines
    in repr, every 7th in E-notation (both read back bit for bit); each maximal fan run (a, b, c), (a, c, d), (a, d, e) ...
    as ONE polygon (`f a b c d e ...`); corners as `a`, `a//n`, `a/t/n`, `a/t` in turn, every 3rd polygon with negative
    (relative) indices, every 5th with a run of blanks after `f`; after every `degenerate_every`-th polygon (0: never) a
    zero-area quad `f a a b b` (two zero-area fan triangles); no final newline.  Returns (path, injected triangles)."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces)
    nv = len(v)
    lines = ["# %d vertices, %d triangles" % (nv, len(f)), "mtllib m.mtl", "o obj"]
    lines += [("v " + " ".join(("%.16E" if k % 7 == 3 else "%r") % float(x) for x in p)) for k, p in enumerate(v)]
    lines += ["vn 0.0 0.0 1.0", "vt 0.5 0.5", "s off", "g grp", "usemtl m"]
    polys, k = [], 0
    while k < len(f):
        poly = [int(i) for i in f[k]]
        k += 1
        while k < len(f) and f[k][0] == poly[0] and f[k][1] == poly[-1]:
            poly.append(int(f[k][2]))
            k += 1
        polys.append(poly)
    forms = ("%d", "%d//1", "%d/1/1", "%d/1")
    injected = 0
    for j, poly in enumerate(polys):
        idx = [i - nv if j % 3 == 2 else i + 1 for i in poly]
        lines.append("f" + ("     " if j % 5 == 4 else " ") + " ".join(forms[j % 4] % i for i in idx))
        if degenerate_every and j % degenerate_every == degenerate_every - 1:
            lines.append("f %d %d %d %d" % (poly[0] + 1, poly[0] + 1, poly[1] + 1, poly[1] + 1))
            injected += 2
        if j % 500 == 499:
            lines.append("usemtl m")
    with open(path, "w") as fh:
        fh.write("\n".join(lines))
    return str(path), injected


def share_an_edge(tri_a, tri_b, tol=1e-9):
    """Two triangles ([3, 3] vertex arrays) with at least two common vertices."""
    common = sum(1 for p in tri_a if np.any(np.all(np.abs(tri_b - p) <= tol * (1.0 + np.abs(p).max()), axis=1)))
    return common >= 2


def check_hits_against_fixture(prim, t, fix_prim, fix_t, fix_second, tris, rtol=1e-12):
    """Nearest hits (triangle index into `tris`, distance) against a brute-force fixture.  Index and decision work is
    exact: a differing triangle is accepted ONLY as a tie -- the same distance to rtol on two triangles that share an
    edge (the ray passes through the common edge; which of the two claims it is decided in the last bit)."""
    assert np.array_equal(prim >= 0, fix_prim >= 0), "hit / miss decisions differ"
    hit = fix_prim >= 0
    np.testing.assert_allclose(t[hit], fix_t[hit], rtol=rtol)
    diff = np.flatnonzero(hit & (prim != fix_prim))
    for i in diff:
        assert abs(fix_second[i] - fix_t[i]) <= 1e-9 * fix_t[i], "ray %d: another triangle although the hit is not a tie" % i
        assert share_an_edge(tris[prim[i]], tris[fix_prim[i]]), "ray %d: tie between triangles that share no edge" % i
    return len(diff)


# ---------------------------------------------------------------- surface renderers (lt_render_surface / _old)
RENDER_LDS_BUDGET = 48 * 1024      # launch_render_surface stages the scene tables in LDS up to this many bytes


def render_table_bytes(n_tris, n_nodes):
    """The bytes of scene tables k_render_surface<true> stages in LDS (launch_render_surface): per triangle a TriD<double>
    (104 B) and an lt_surface_material (64 B), per node a NodeD<double> (64 B) and 8 x 2 int16 links (32 B)."""
    return n_tris * (104 + 64) + n_nodes * 64 + (16 * n_nodes * 2 + 3) // 4 * 4


def cone_mesh():
    """(vertices, faces) of the notebook's cone (cornell_box.get_cone, 10 triangles)."""
    tris = cb.get_cone(K.GLASS_MAT)
    v = np.concatenate([t.vertices3() for t in tris])
    return v, np.arange(len(v)).reshape(-1, 3)


def render_scene(verts, faces, half=7.5, fill=0.8, glass_every=3, n_light_samples=16, seed=3, split_method=0):
    """A vertex / face mesh in the notebook's open Cornell box (cornell_box.get_cornell_box + get_light_quad, no front
    wall: the camera looks in), turned so that its thinnest side faces the camera, scaled so that its longest side is
    `fill` of the box and centred, SAH-built.  Materials reach every branch of both integrators: diffuse walls (coloured
    left / right, grey floor and ceiling), a MIRROR back wall, the light quad (diffuse, is_light, emission 200), and the
    object's faces split between GLASS (transmission 1, ior 1.5; every `glass_every`-th face) and dark diffuse ones, which
    absorb most of what reaches them so that roulette ends deep paths.  Point lights: 2 x n_light_samples samples of the
    light quad (generate_area_light_samples).
    Returns dict(mesh (set_mesh arrays), mats [T, 9] rows as oracle.render_surface takes them, lights [L, 10],
    camera, f_distance, is_object [T] bool, n_tris, n_nodes)."""
    from light_transport_amd.src.io import triangles_from_mesh
    from light_transport_amd.src.light_samples import generate_area_light_samples
    from light_transport_amd.src.material import Material
    v = np.asarray(verts, dtype=np.float64)
    thin = int(np.argmin(v.max(axis=0) - v.min(axis=0)))
    v = np.roll(v, 2 - thin, axis=1)        # (a rotation) its thinnest side towards the camera: the wine glass lies flat
    lo, hi = v.min(axis=0), v.max(axis=0)
    scale = fill * 2 * half / float((hi - lo).max())
    shift = -0.5 * (lo + hi) * scale
    src = Material(color=K.WHITE, shininess=1, reflection=0.9, ior=1.5, emission=200)
    box = cb.get_cornell_box(half, K.GLASS_MAT, K.GLASS_MAT, K.GLASS_MAT)
    lq = cb.get_light_quad(half, src)
    roles = ["right"] * 2 + ["left"] * 2 + ["mirror"] * 2 + ["grey"] * 10
    for t, r in zip(box, roles):
        t.role = r
    for t in lq:
        t.role = "light"
    body = triangles_from_mesh(v, faces, K.GLASS_MAT, scale, shift, drop_degenerate=False)
    for k, t in enumerate(body):
        t.role = "glass" if k % glass_every == 0 else "dark"
    ordered, linear = B.build_linear_bvh(box + lq + body, split_method)
    row = {  # diffuse[3], emission, ior, transmission, is_diffuse, is_mirror, is_light
        "right": [0.0, 0.6, 0.0, 0, 1.5, 0, 1, 0, 0], "left": [0.7, 0.0, 0.0, 0, 1.5, 0, 1, 0, 0],
        "grey": [0.55, 0.55, 0.55, 0, 1.5, 0, 1, 0, 0], "mirror": [0.9, 0.9, 0.9, 0, 1.5, 0, 0, 1, 0],
        "light": [1.0, 1.0, 1.0, 200, 1.5, 0, 1, 0, 1], "glass": [0.6, 0.7, 0.7, 0, 1.5, 1, 0, 0, 0],
        "dark": [0.15, 0.2, 0.25, 0, 1.5, 0, 1, 0, 0]}
    mats = np.array([row[t.role] for t in ordered], dtype=np.float64)
    np.random.seed(seed)
    lights = np.array([list(l.source[:3]) + list(l.normal[:3]) + [l.material.emission * x for x in l.material.color.diffuse[:3]]
                       + [l.total_area] for l in generate_area_light_samples(lq[0], lq[1], src, n_light_samples, 4)])
    mesh = dict(verts=B.triangles_array(ordered), med_front=-np.ones(len(ordered), np.int32),
                med_back=-np.ones(len(ordered), np.int32), nodes=B.linear_bvh_arrays(linear))
    # the screen (x, y in [-1, 1] x [-1 / aspect, 1 / aspect]) one unit in front of a camera just outside the open side:
    # a 90-degree view in which the object fills the middle and walls, mirror and light show around it
    return dict(mesh=mesh, mats=mats, lights=lights, camera=np.array([0.0, 0.0, half + 0.5]), f_distance=half - 0.5,
                is_object=np.array([t.role in ("glass", "dark") for t in ordered]), n_tris=len(ordered),
                n_nodes=len(mesh["nodes"]["offset"]))


def render_tables(W, H, S, D, n_lights, choices=None, seed=0):
    """Seeded tables of one render: xs [W], ys [H] (np.linspace of the Scene's left..right / top..bottom), rand_0, rand_1
    [H][W][S][D] and light_choice -- [H][W][S][D] for lt_render_surface, [H][W][S][choices] for lt_render_surface_old.
    Every entry is an independent draw."""
    rs = np.random.RandomState(seed)
    r0, r1 = rs.rand(H, W, S, D), rs.rand(H, W, S, D)
    lc = rs.randint(0, n_lights, size=(H, W, S, D if choices is None else choices)).astype(np.int32)
    xs, ys = np.linspace(-1, 1, W), np.linspace(1 / (W / H), -1 / (W / H), H)
    return xs, ys, r0, r1, lc


def camera_rays(sc, xs, ys, rand_0):
    """The bounce-0 rays of every (pixel, sample) (path_tracing_fix1.py:152-160: the jitter re-uses rand_0[..., 0])."""
    H, W, S, _ = rand_0.shape
    jit = rand_0[..., 0]
    cam = sc["camera"]
    d = np.stack([xs[None, :, None] + jit / W - cam[0], ys[:, None, None] + jit / H - cam[1],
                  np.full((H, W, S), sc["f_distance"] - cam[2])], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.broadcast_to(cam, d.shape).copy(), d
