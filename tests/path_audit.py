"""Audit captured photon paths event by event against the raw random draws they consumed.

A plain helper (no conftest, no fixtures).  It imports neither the oracle nor the product package: callers hand it the scene
as plain data, the raw 32-bit draws of every photon, the captured vertex records, the counters and the tally.  Everything is
re-derived in np.longdouble (>= 64-bit mantissa) from textbook laws -- the exponential free path, the Henyey-Greenstein CDF,
Snell's law, Fresnel's angle forms, the MCML rotation frame -- so an error that the walk kernels and the CPU oracle share
(both were written from the same appendix) shows up here.

    scene = dict(media=[(mu_a, mu_s, g, n), ...],
                 layers=dict(z_bounds, medium_idx, n_above, n_below) | None,
                 mesh=dict(verts [T, 3, 3], med_front [T], med_back [T]) | None,
                 source=dict(type, pos, dir, extra, start_medium),
                 grid=dict(shape=(nx, ny, nz), origin, voxel), quantity=0 | 1, max_steps=K - 1,
                 roulette_factor=10)                              # optional; the mutation tests change it
    audit(scene, draws uint32 [n, 4 G], vertices [n, K], counts [n], counters, grid, grid_kind="f64" | "u64fx", tol=None)

returns {check: dict(worst={measure: value}, n=events, violations=int, declined=int, ...)} for the checks A..J of the module
that calls it (tests/test_path_audit_cpu.py lists them).  A deviation above TOL[measure] and every discrete mismatch (a
kind, a medium, a step count) is a violation.

Facts of the walk the audit relies on (include/lt.h, lt_walk_kernel.inc): a uniform is (k + 1) 2^-32 of one raw draw k;
step s (vertex field step = s + 1) consumes draw group s (s + 1 behind a cosine-quad source, whose emission takes group 0);
within a group u0 is the free path, u1 the deflection, u2 the azimuth, u3 the interface decision or the roulette; every step
that does not end the path silently leaves exactly one vertex; `direction` is the direction on ARRIVAL.

Designed rules of the walk, stated here and not exempted silently:
  * |uz| > 0.99999 before a scattering: the new direction is (sin t cos p, sin t sin p, sign(uz) cos t),
    an approximation unless |uz| = 1; C and D apply this rule there, count the approximated events in C["pole"] (the callers
    cap their frequency) and those exactly on the axis in C["axis"].
  * after a mesh event the point is pushed 1e-6 along the facing normal (reflection) or against it (transmission); a
    triangle is seen only beyond t > 1e-6 and at |d.n| > 1e-7.  Hits the rule hides are counted in G["hidden"].
  * the weight roulette: below 1e-4 a path survives with probability 0.1 and ten times the weight.
"""
import itertools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the audit needs an extended-precision long double"

LIGHT, REFLECTIVE, TRANSMISSIVE, VOLUME = 5, 3, 4, 7           # include/lt.h: LT_VERTEX_*
SRC_PENCIL, SRC_COSINE_QUAD = 0, 1
PUSH = LD(np.float64(1e-6))          # the walk's epsilon: push after a mesh event, emission offset, nearest admissible hit
GRAZING = 1e-7                       # |d.n| below which the walk does not see a triangle
POLE = np.float64(0.99999)
ROULETTE_BELOW, ROULETTE_CHANCE = LD(np.float64(1e-4)), LD(np.float64(0.1))
DECLINE_U3 = LD(10) ** -12           # |u3 - R| below which a reflect / transmit decision is too close to call
FACE_BAND = LD(10) ** -9             # a deposit this close (in voxels) to a voxel face may count to either neighbour
PI = 4 * np.arctan(LD(1))
COUNTERS = ("w_absorbed", "w_lost_outside_grid", "w_escaped_top", "w_escaped_bottom", "w_escaped_mesh", "w_specular",
            "w_roulette_net", "w_capped")

# The CPU oracle's worst deviation per measure over the scenes of tests/path_audit_scenes.py (seed 97), rounded up to two
# digits; tests/test_path_audit_cpu.py asserts that the oracle stays within them.  A tolerance is 16 x that, rounded up to a
# power of ten (the factor covers the kernels' lean reciprocal, rsqrt and polynomial forms), and never above 1e-8.
# Not measured but derived: F.reflect is exact (a sign flip); G.inside takes G.plane's figure -- both are the distance of the
# recorded double-precision point from the triangle, across its plane and within it; I.sum and J.voxel are ratios to the
# rounding-error bounds derived where they are computed, so their tolerance is 1.
ORACLE_WORST = {
    "A.tau": 1.2e-11, "B.perp": 1.7e-15, "B.unit": 3.4e-12, "C.cdf": 6.2e-13, "D.azimuth": 1.1e-12, "E.weight": 1.2e-16,
    "E.pdf": 3.5e-12, "F.R": 3.7e-13, "F.snell": 5.5e-15, "F.plane": 5.5e-17,
    "G.plane": 3.1e-16, "G.nearest": 5.6e-14, "G.normal": 9.1e-17, "G.R": 8.9e-14, "G.reflect": 3.8e-16, "G.snell": 1.5e-14,
    "G.plane_of_incidence": 1.1e-16, "H.point": 4.5e-16, "H.dir": 1.5e-15, "H.weight": 4.8e-17, "H.pdf": 3.9e-16,
}


def tolerance(worst):
    return min(1e-8, 10.0 ** int(np.ceil(np.log10(16.0 * worst) - 1e-12)))


def _tolerances(worst):
    t = {k: tolerance(w) for k, w in worst.items()}
    if "E.pdf_roundings" in worst:      # a ratio (to the effect of one rounding of the cosine): the same rule without the cap
        t["E.pdf_roundings"] = 10.0 ** int(np.ceil(np.log10(16.0 * worst["E.pdf_roundings"]) - 1e-12))
    t.update({"F.reflect": 0.0, "G.inside": t["G.plane"], "I.sum": 1.0, "J.voxel": 1.0})
    return t


# The same for the scenes at the edges of the medium parameters (path_audit_scenes.EDGE; measured after the walk's tiny-g fix):
# their own table, so that the scenes above keep the tolerances they have always had.  Entries are the oracle's worst over the
# edge scenes where that exceeds the figure above (the sliver layer and the near-matched indices: Snell and Fresnel between
# nearly equal indices; the cone of scene t_g1e-6_cone), and the measures only those scenes have:
#   C.cos            |g| >= 0.99: the cosine's deviation from the exact inverse CDF where the CDF's deviation exceeds TOL[C.cdf]
#   E.pdf_roundings  |g| >= 0.99: the HG value's deviation in roundings of the cosine where it exceeds TOL[E.pdf]
#   E.weight_in      albedo < 2^-10: the surviving weight's deviation in units of the weight that came in
ORACLE_WORST_EDGE = dict(ORACLE_WORST, **{
    "F.R": 5.1e-13, "F.plane": 6.7e-17, "F.snell": 5.8e-14, "G.plane": 4.5e-16, "G.snell": 5.5e-14, "H.weight": 7.1e-17,
    "C.cos": 1.9e-16, "E.pdf_roundings": 1.2, "E.weight_in": 7.7e-17,
})

TOL = _tolerances(ORACLE_WORST)
TOL_EDGE = _tolerances(ORACLE_WORST_EDGE)
TOL.update({k: TOL_EDGE[k] for k in ("C.cos", "E.pdf_roundings", "E.weight_in")})      # (no scene above has such a medium)


class _Check:
    def __init__(self, name, tol):
        self.name, self.tol = name, tol
        self.worst, self.n, self.violations, self.declined, self.extra = {}, 0, 0, 0, {}

    def measure(self, what, dev, count=True):
        """dev: deviations of the events checked (any shape); those above the tolerance are violations."""
        dev = np.asarray(dev, dtype=LD).ravel()
        if dev.size == 0:
            self.worst.setdefault(what, 0.0)
            return
        if count:
            self.n += dev.size
        bad = ~(dev <= LD(self.tol[what]))          # (NaN is a violation)
        self.violations += int(bad.sum())
        self.worst[what] = max(self.worst.get(what, 0.0), float(np.nanmax(dev)) if not np.all(np.isnan(dev)) else np.inf)

    def require(self, ok):
        self.violations += int((~np.asarray(ok, dtype=bool)).sum())

    def result(self):
        return dict(worst=dict(self.worst), n=self.n, violations=self.violations, declined=self.declined, **self.extra)


def uniforms(draws, groups):
    """[n, groups, 4] uniforms in (0, 1] of raw 32-bit draws [n, >= 4 groups]: u = (k + 1) 2^-32."""
    d = np.asarray(draws)
    assert d.dtype == np.uint32 and d.ndim == 2 and d.shape[1] >= 4 * groups
    return ((d[:, :4 * groups].astype(LD) + 1) * LD(2) ** -32).reshape(d.shape[0], groups, 4)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def fresnel_angle_form(sin_i, cos_i, n1, n2):
    """Unpolarised reflectance from the angle forms R = [sin^2(i - t) / sin^2(i + t) + tan^2(i - t) / tan^2(i + t)] / 2 with
    t from Snell's law; ((n1 - n2) / (n1 + n2))^2 at normal incidence, 1 beyond the critical angle, 0 between equal indices."""
    sin_i, cos_i, n1, n2 = np.broadcast_arrays(*(np.asarray(x, dtype=LD) for x in (sin_i, cos_i, n1, n2)))
    ti = np.arctan2(sin_i, cos_i)
    st = n1 * sin_i / n2
    tt = np.arcsin(np.minimum(st, LD(1)))
    with np.errstate(all="ignore"):
        r = (np.sin(ti - tt) ** 2 / np.sin(ti + tt) ** 2 + np.tan(ti - tt) ** 2 / np.tan(ti + tt) ** 2) / 2
    r = np.where(sin_i == 0, ((n1 - n2) / (n1 + n2)) ** 2, r)
    r = np.where(st >= 1, LD(1), r)
    return np.where(n1 == n2, LD(0), r)


def hg_cdf(c, g):
    """P(cos <= c) of the Henyey-Greenstein phase function in the deflection-angle convention (g > 0: forward), in the form
    (1 - g)(1 + c) / (D (1 + g + D)), D = sqrt(1 + g^2 - 2 g c): the textbook (1 - g^2) / (2 g) (1 / D - 1 / (1 + g)) with its
    difference multiplied out.  Nothing cancels and nothing divides by g, so it holds at g = 0 ((1 + c) / 2) and at
    g = 1e-12, where the textbook form is good to 5e-20 / |g| = 5e-8 even in long double."""
    c, g = np.broadcast_arrays(np.asarray(c, dtype=LD), np.asarray(g, dtype=LD))
    with np.errstate(all="ignore"):
        d = np.sqrt(1 + g * g - 2 * g * c)
        return (1 - g) * (1 + c) / (d * (1 + g + d))


def hg_inverse(u, g):
    """The cosine whose hg_cdf is u.  |g| < 0.5: s + g (1 - s^2)(3 + 2 g s - g^2) / (2 (1 + g s)^2) with s = 2 u - 1, the
    textbook ((1 + g^2) - t^2) / (2 g), t = (1 - g^2) / (1 - g + 2 g u), rearranged so that nothing cancels as g -> 0 (the
    two agree to 1e-18 in long double at g = 0.1 .. 0.9); the textbook form beyond, where it is the better conditioned one."""
    u, g = np.broadcast_arrays(np.asarray(u, dtype=LD), np.asarray(g, dtype=LD))
    s = 2 * u - 1
    small = s + g * (1 - s * s) * (3 + 2 * g * s - g * g) / (2 * (1 + g * s) ** 2)
    gs = np.where(np.abs(g) < 0.5, LD(1), g)
    with np.errstate(all="ignore"):
        t = (1 - gs * gs) / (1 - gs + 2 * gs * u)
        text = (1 + gs * gs - t * t) / (2 * gs)
    return np.where(np.abs(g) < 0.5, small, text)


def hg_pdf(c, g):
    c, g = np.broadcast_arrays(np.asarray(c, dtype=LD), np.asarray(g, dtype=LD))
    d = 1 + g * g - 2 * g * c
    return (1 - g * g) / (4 * PI * d * np.sqrt(d))


def _ray_triangles(O, Dr, tmax, A, AB, AC, budget=4000000):
    """All (ray, triangle) pairs that may intersect up to tmax (+ margin), brute force over every pair: bounding boxes and
    float64 Moller-Trumbore as prefilters with generous margins, then long double on the candidates.  Returns ray index, triangle index, t, u, v, d.n."""
    M, T = O.shape[0], A.shape[0]
    O64, D64, A64, AB64, AC64 = (np.asarray(x, dtype=np.float64) for x in (O, Dr, A, AB, AC))
    t64 = np.asarray(tmax, dtype=np.float64)
    scale = max(1.0, float(np.abs(A64).max()) if T else 1.0)
    ri, ti = [], []
    step = max(1, budget // max(T, 1))
    m = 1e-6
    corners = np.stack([A64, A64 + AB64, A64 + AC64])
    tlo, thi = corners.min(axis=0) - m * scale, corners.max(axis=0) + m * scale
    E64 = O64 + D64 * t64[:, None]
    slo, shi = np.minimum(O64, E64), np.maximum(O64, E64)
    for lo in range(0, M, step):                       # boxes first: a segment meets few triangles' boxes
        r, k = np.nonzero(((slo[lo:lo + step, None, :] <= thi[None]) & (shi[lo:lo + step, None, :] >= tlo[None])).all(axis=-1))
        r += lo
        o, d = O64[r], D64[r]
        pv = np.cross(d, AC64[k])
        det = (AB64[k] * pv).sum(-1)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = o - A64[k]
            u = (tv * pv).sum(-1) * inv
            qv = np.cross(tv, AB64[k])
            v = (d * qv).sum(-1) * inv
            t = (AC64[k] * qv).sum(-1) * inv
        cand = (np.abs(det) > 0) & (u > -m) & (v > -m) & (u + v < 1 + m) & (t > -m * scale) & (t < t64[r] + m * scale)
        ri.append(r[cand]); ti.append(k[cand])
    ri = np.concatenate(ri) if ri else np.zeros(0, np.int64)
    ti = np.concatenate(ti) if ti else np.zeros(0, np.int64)
    o, d, a, ab, ac = O[ri], Dr[ri], A[ti], AB[ti], AC[ti]
    pv = _cross(d, ac)
    det = _dot(ab, pv)
    tv = o - a
    qv = _cross(tv, ab)
    with np.errstate(all="ignore"):
        u, v, t = _dot(tv, pv) / det, _dot(d, qv) / det, _dot(ac, qv) / det
    nrm = _cross(ab, ac)
    nrm = nrm / _norm(nrm)[:, None]
    return ri, ti, t, u, v, _dot(d, nrm)


def audit(scene, draws, vertices, counts, counters, grid, grid_kind="f64", tol=None):
    tol = dict(TOL, **(tol or {}))
    chk = {c: _Check(c, tol) for c in "ABCDEFGHIJ"}
    v, cnt = vertices, np.asarray(counts).astype(np.int64)
    n, K = v.shape
    media = np.array(scene["media"], dtype=LD).reshape(-1, 4)
    mu_a, mu_t, g_m, n_m = media[:, 0], media[:, 0] + media[:, 1], media[:, 2], media[:, 3]
    with np.errstate(all="ignore"):
        absorb = np.where(mu_t > 0, mu_a / mu_t, LD(0))
        inv_mu_t = np.where(mu_t > 0, 1 / mu_t, LD(0))
    layers, mesh, src = scene.get("layers"), scene.get("mesh"), scene["source"]
    layered = layers is not None
    max_steps = int(scene["max_steps"])
    assert max_steps == K - 1, "run every scene with max_steps = K - 1, so that every path is captured whole"
    factor = LD(scene.get("roulette_factor", 10))
    quad = int(src.get("type", 0)) == SRC_COSINE_QUAD
    goff = 1 if quad else 0
    G = K + 1
    U = uniforms(draws, G)

    P, D, Wt = v["point"].astype(LD), v["direction"].astype(LD), v["throughput"].astype(LD)
    kind, med, step = v["kind"].astype(np.int64), v["medium"].astype(np.int64), v["step"].astype(np.int64)
    pdf_dir, gn = v["pdf_dir"].astype(LD), v["g_norm"].astype(LD)
    jj = np.arange(K)[None, :]
    live = jj < cnt[:, None]
    nxt_live = np.zeros_like(live); nxt_live[:, :-1] = live[:, 1:]              # vertex j + 1 exists
    is_vol, is_if = live & (kind == VOLUME), live & ((kind == REFLECTIVE) | (kind == TRANSMISSIVE))
    is_light = live & (kind == LIGHT)
    I, J = chk["I"], chk["J"]
    # every step leaves exactly one vertex: vertex j is the event of step j - 1; kinds are the four known ones
    I.require((step == jj)[live]); I.require((is_light == (live & (jj == 0)))); I.require((is_vol | is_if | is_light)[live])
    I.require(cnt >= 1)
    step = np.where(live, np.clip(step, 0, K - 1), 0)
    grp = np.clip(step - 1 + goff, 0, G - 1)                                   # the draw group of the step that made vertex j
    Ug = np.take_along_axis(U, grp[:, :, None], axis=1)                        # [n, K, 4]
    u1, u2, u3 = Ug[..., 1], Ug[..., 2], Ug[..., 3]

    if layered:
        zb = np.array(layers["z_bounds"], dtype=LD)
        lm = np.asarray(layers["medium_idx"], dtype=np.int64)
        nl = len(lm)
        lay = np.clip(med, 0, nl - 1)
        I.require((med == lay)[live])
        mid = lm[lay]                                                          # medium id on arrival
    else:
        mid = np.clip(med, 0, len(media) - 1)
        I.require((med == mid)[live])
    Dn = _norm(D)
    with np.errstate(all="ignore"):
        Du = D / Dn[..., None]                                                 # unit directions

    # ---------------------------------------------------------------- interfaces: what the event must have done
    refl_exp = np.zeros((n, K), bool)      # the event reflects
    gone = np.zeros((n, K), bool)          # the event transmits out of the scene
    med_after = med.copy()                 # layer / medium id in which the path goes on
    push = np.zeros((n, K, 3), dtype=LD)
    nf_if = np.zeros((n, K, 3), dtype=LD)  # facing normal of the interface
    n1a, n2a = np.ones((n, K), dtype=LD), np.ones((n, K), dtype=LD)
    Rf = np.zeros((n, K), dtype=LD)
    F, Gc = chk["F"], chk["G"]
    if layered:
        down = D[..., 2] > 0
        bound = np.where(down, zb[np.clip(lay + 1, 0, nl)], zb[lay])
        F.require((P[..., 2] == bound)[is_if])                                 # snapped onto the bound, exactly
        F.require((D[..., 2] != 0)[is_if])
        nxt = np.where(down, lay + 1, lay - 1)
        outside = (nxt < 0) | (nxt >= nl)
        n1a = n_m[mid]
        n2a = np.where(nxt < 0, LD(layers.get("n_above", 1.0)), np.where(nxt >= nl, LD(layers.get("n_below", 1.0)),
                                                                          n_m[lm[np.clip(nxt, 0, nl - 1)]]))
        sin_i, cos_i = np.sqrt(Du[..., 0] ** 2 + Du[..., 1] ** 2), np.abs(Du[..., 2])
        nf_if[..., 2] = np.where(down, LD(-1), LD(1))
        if_chk = F
    else:
        A = np.asarray(mesh["verts"], dtype=LD).reshape(-1, 3, 3)
        tA, tAB, tAC = A[:, 0], A[:, 1] - A[:, 0], A[:, 2] - A[:, 0]
        mf, mb = np.asarray(mesh["med_front"], dtype=np.int64), np.asarray(mesh["med_back"], dtype=np.int64)
        # the push of vertex j - 1 is needed before its own event is audited: take it from the recorded facing normal
        # (g_norm), which G.normal then compares with the normal of the triangle the audit itself finds
        sgn = np.where(kind == REFLECTIVE, LD(1), LD(-1))
        push = np.where(is_if[..., None], sgn[..., None] * PUSH * gn, LD(0))
        if_chk = Gc
    start = P + push
    seg = live & (jj >= 1)                                                     # segment j - 1 -> j
    delta = np.zeros_like(P); delta[:, 1:] = P[:, 1:] - start[:, :-1]
    seglen = _norm(delta)

    if not layered:
        si, sj = np.nonzero(seg)
        ri, ti, t, u, vv, ddn = _ray_triangles(start[si, sj - 1], D[si, sj], seglen[si, sj], tA, tAB, tAC)
        ln = seglen[si, sj][ri]
        seen = np.abs(ddn) > GRAZING
        inside = (u >= 0) & (vv >= 0) & (u + vv <= 1)
        margin = LD(10) ** -9
        interior = (u > margin) & (vv > margin) & (u + vv < 1 - margin)
        # the leak check: no segment crosses the interior of a triangle the walk can see before its end
        leak = interior & seen & (t > PUSH * (1 + margin)) & (t < ln - margin * (1 + ln))
        Gc.extra["leaks"] = int(leak.sum())
        Gc.violations += int(leak.sum())
        Gc.extra["hidden"] = int((inside & (t > 0) & (t < ln - margin * (1 + ln)) & ~(seen & (t > PUSH))).sum())
        Gc.extra["segments"] = len(si)
        # the event triangle of an interface vertex: the admissible hit nearest to the recorded point
        ev = is_if[si, sj][ri]
        near = ev & seen & (u >= -margin) & (vv >= -margin) & (u + vv <= 1 + margin) & (t > PUSH * (1 - margin))
        score = np.where(near, np.abs(t - ln), np.inf)
        order = np.lexsort((score.astype(np.float64), ri))
        first = np.ones(len(order), bool); first[1:] = ri[order][1:] != ri[order][:-1]
        best = order[first]
        best = best[near[best]]
        tri_of = -np.ones((n, K), np.int64)
        tri_of[si[ri[best]], sj[ri[best]]] = ti[best]
        t_of = np.full((n, K), np.nan, dtype=LD); t_of[si[ri[best]], sj[ri[best]]] = t[best]
        Gc.require((tri_of >= 0)[is_if])                                       # the point lies on a triangle ahead
        Gc.extra["tri_events"] = np.bincount(tri_of[is_if & (tri_of >= 0)], minlength=len(tA))     # events per triangle
        ok = is_if & (tri_of >= 0)
        tk = np.clip(tri_of, 0, None)
        N = _cross(tAB, tAC)
        nrm_t = N / _norm(N)[:, None]
        nrm = nrm_t[tk]
        w = P - tA[tk]
        NN = _dot(N, N)[tk]
        with np.errstate(all="ignore"):
            bu, bv = _dot(_cross(w, tAC[tk]), N[tk]) / NN, _dot(_cross(tAB[tk], w), N[tk]) / NN
        Gc.measure("G.plane", np.abs(_dot(w, nrm))[ok])
        # (how far outside the triangle, as a length: the same error of the recorded point as G.plane, within the plane)
        edge = np.maximum(_norm(tAB), _norm(tAC))[tk]
        Gc.measure("G.inside", (np.maximum(np.maximum(-bu, -bv), np.maximum(bu + bv - 1, 0)) * edge)[ok].clip(0), count=False)
        Gc.measure("G.nearest", np.abs(t_of - seglen)[ok], count=False)
        # a second admissible triangle at the same distance that would change the event: too close to call
        same = near & (np.abs(t - t_of[si, sj][ri]) < margin) & (ti != tri_of[si, sj][ri])
        if same.any():
            a_, b_ = ti[same], tri_of[si, sj][ri][same]
            differ = (np.abs(_dot(nrm_t[a_], nrm_t[b_])) < 1 - margin) | (mf[a_] != mf[b_]) | (mb[a_] != mb[b_])
            Gc.declined += int(differ.sum())
        dn = _dot(Du, nrm)
        nf_if = np.where((dn > 0)[..., None], -nrm, nrm)
        Gc.measure("G.normal", np.abs(gn - nf_if).max(axis=-1)[ok], count=False)
        nxt = np.where(dn > 0, mf[tk], mb[tk])
        outside = nxt < 0
        n1a = n_m[mid]
        n2a = np.where(outside, n1a, n_m[np.clip(nxt, 0, len(media) - 1)])     # the exterior is index matched
        sin_i, cos_i = _norm(_cross(Du, nrm)), np.abs(dn)

    Rf = fresnel_angle_form(sin_i, cos_i, n1a, n2a)
    refl_exp = is_if & (u3 <= Rf)
    declined = is_if & (np.abs(u3 - Rf) < DECLINE_U3)
    if_chk.declined += int(declined.sum())
    if_chk.require(((kind == REFLECTIVE) == refl_exp)[is_if & ~declined])
    refl = is_if & (kind == REFLECTIVE)            # from here on follow the recorded branch (a wrong one is counted above)
    trans = is_if & ~refl
    gone = trans & outside
    med_after = np.where(trans, nxt, med)
    Rname = "F.R" if layered else "G.R"
    if_chk.measure(Rname, np.abs(pdf_dir - np.where(gone, LD(0), np.where(refl, Rf, 1 - Rf)))[is_if], count=layered)
    if_chk.require(~(gone & nxt_live))                                         # a path that left has no further vertex
    if_chk.extra.update(reflected=int(refl.sum()), transmitted=int((trans & ~gone).sum()), left=int(gone.sum()), crossed=int(trans.sum()),
                        total_internal=int((refl & (Rf >= 1)).sum()), events=int(is_if.sum()))
    # the direction after the event is the arrival direction of the next vertex; the medium follows the side entered
    Dnext = np.zeros_like(D); Dnext[:, :-1] = D[:, 1:]
    Dunext = np.zeros_like(D); Dunext[:, :-1] = Du[:, 1:]
    mednext = np.zeros_like(med); mednext[:, :-1] = med[:, 1:]
    if_chk.require((mednext == med_after)[nxt_live & live])
    a, b = refl & nxt_live, trans & nxt_live & ~gone
    if layered:
        F.measure("F.reflect", np.abs(Dnext - D * np.array([1, 1, -1], dtype=LD)).max(axis=-1)[a], count=False)
        s_t = np.sqrt(Dunext[..., 0] ** 2 + Dunext[..., 1] ** 2)
        F.measure("F.snell", np.abs(n1a * sin_i - n2a * s_t)[b], count=False)
        F.measure("F.plane", np.abs(Du[..., 0] * Dunext[..., 1] - Du[..., 1] * Dunext[..., 0])[b], count=False)
        F.require(((Dnext[..., 2] > 0) == (D[..., 2] > 0))[b])
        F.require((Du[..., 0] * Dunext[..., 0] + Du[..., 1] * Dunext[..., 1] >= 0)[b])
    else:
        dnf = _dot(Du, nf_if)
        Gc.measure("G.reflect", np.abs(Dunext - (Du - 2 * dnf[..., None] * nf_if)).max(axis=-1)[a], count=False)
        Gc.measure("G.snell", np.abs(n1a * sin_i - n2a * _norm(_cross(Dunext, nf_if)))[b], count=False)
        Gc.measure("G.plane_of_incidence", np.abs(_dot(Dunext, _cross(Du, nf_if)))[b], count=False)
        Gc.require((_dot(Dunext, nf_if) < 0)[b])
        tan_i, tan_t = Du - dnf[..., None] * nf_if, Dunext - _dot(Dunext, nf_if)[..., None] * nf_if
        Gc.require((_dot(tan_i, tan_t) >= 0)[b])

    # ---------------------------------------------------------------- A: free path
    A_ = chk["A"]
    anchor = is_vol | is_light
    last_anchor = np.maximum.accumulate(np.where(anchor, jj, 0), axis=1)       # latest anchor at or before j
    prev_anchor = np.zeros_like(last_anchor); prev_anchor[:, 1:] = last_anchor[:, :-1]
    tau_seg = np.where(seg, seglen * mu_t[mid], LD(0))                         # (vertex j's medium is the segment's)
    csum = np.cumsum(tau_seg, axis=1)
    tau = csum - np.take_along_axis(csum, prev_anchor, axis=1)
    g_draw = np.clip(np.take_along_axis(step, prev_anchor, axis=1) + goff, 0, G - 1)   # the step after the anchor drew
    u0 = np.take_along_axis(U[..., 0], g_draw, axis=1)
    sel = is_vol & (jj >= 1)
    A_.measure("A.tau", np.abs(tau + np.log(u0))[sel])
    A_.extra["carried"] = int((sel & (prev_anchor < jj - 1)).sum())            # free paths carried through >= 1 interface
    A_.extra["through_clear"] = int((is_if & (mu_t[mid] == 0)).sum())

    # ---------------------------------------------------------------- B: straight segments, unit directions
    B_ = chk["B"]
    B_.measure("B.perp", _norm(_cross(delta, Du))[seg])
    B_.measure("B.unit", np.abs(Dn - 1)[live], count=False)
    B_.require((_dot(delta, D) > 0)[seg & (seglen > 0)])

    # ---------------------------------------------------------------- C, D: deflection and azimuth at a scattering
    C_, D_ = chk["C"], chk["D"]
    sc = is_vol & nxt_live
    uz = v["direction"][..., 2]
    pole = np.abs(uz) > POLE
    sgn_z = np.where(uz >= 0, LD(1), LD(-1))
    c = np.where(pole, sgn_z * Dunext[..., 2], _dot(Du, Dunext))
    gg = g_m[mid]
    # |g| >= 0.99: the CDF is ill-conditioned in the cosine (dCDF / dc reaches (1 + g) / (2 (1 - g)^2), 1e6 at g = 0.999: a
    # cosine good to one rounding is 1e-10 off in the CDF), and towards the far pole the cosine is ill-conditioned in the CDF.
    # An event there passes when EITHER deviation is within its tolerance: C.cos is the cosine's deviation from the exact
    # inverse of u1 where the CDF's exceeds TOL[C.cdf], 0 elsewhere.  Every other medium keeps the CDF measure alone.
    hard = np.abs(gg) >= LD(0.99)
    cdf_dev = np.abs(hg_cdf(c, gg) - u1)
    C_.measure("C.cdf", cdf_dev[sc & ~hard])
    if (sc & hard).any():
        cos_dev = np.abs(c - hg_inverse(u1, gg))
        C_.measure("C.cos", np.where(cdf_dev <= LD(tol["C.cdf"]), LD(0), cos_dev)[sc & hard])
    # on the axis itself (|uz| = 1, every vertical pencil beam's first scattering) the MCML frame does not exist and the rule
    # IS the rotation, with the azimuth counted from x; between 0.99999 and 1 it is an approximation
    C_.extra["pole"] = int((sc & pole & (np.abs(uz) < 1)).sum())
    C_.extra["axis"] = int((sc & (np.abs(uz) == 1)).sum())
    C_.extra["ill_conditioned"] = int((sc & hard).sum())
    C_.extra["last_medium"] = int((sc & (mid == len(media) - 1)).sum())      # scatterings in the last medium of the table
    with np.errstate(all="ignore"):
        rt = np.sqrt(1 - Du[..., 2] ** 2)
        e1 = np.stack([Du[..., 0] * Du[..., 2], Du[..., 1] * Du[..., 2], -(1 - Du[..., 2] ** 2)], axis=-1) / rt[..., None]
        e2 = np.stack([-Du[..., 1], Du[..., 0], np.zeros_like(rt)], axis=-1) / rt[..., None]
        ca = np.where(pole, Dunext[..., 0], _dot(Dunext, e1))
        cb = np.where(pole, Dunext[..., 1], _dot(Dunext, e2))
    sin_t = np.sqrt(np.maximum(1 - c * c, LD(0)))
    phi = 2 * PI * u2
    D_.measure("D.azimuth", np.maximum(np.abs(ca - sin_t * np.cos(phi)), np.abs(cb - sin_t * np.sin(phi)))[sc])
    D_.extra["pole"] = C_.extra["pole"]

    # ---------------------------------------------------------------- E: weight
    E_ = chk["E"]
    w_after = Wt * (1 - absorb[mid])                                           # after the drop at a scattering
    low = is_vol & (w_after < ROULETTE_BELOW) & (w_after > 0)
    E_.declined += int((is_vol & (np.abs(w_after - ROULETTE_BELOW) < LD(10) ** -17)).sum())
    survives = low & (u3 <= ROULETTE_CHANCE)
    dies = low & ~survives
    w_on = np.where(is_vol, np.where(low, factor * w_after, w_after), Wt)      # weight with which the path goes on
    Wnext = np.zeros_like(Wt); Wnext[:, :-1] = Wt[:, 1:]
    go = live & nxt_live
    with np.errstate(all="ignore"):
        # albedo below 2^-10: what survives the drop, w - w a with a = mu_a / mu_t as a double holds it, is a small difference
        # of the weight that came in -- right to a rounding of THAT (2^-53 w) and no better, whatever the arithmetic, so
        # there the deviation is taken in units of the incoming weight (E.weight_in); everywhere else relative, as ever
        thin_ev = is_vol & ((1 - absorb) < LD(2) ** -10)[mid]
        w_in = Wt * np.where(low, factor, LD(1))
        E_.measure("E.weight", np.abs(Wnext / w_on - 1)[go & ~thin_ev])
        if (go & thin_ev).any():
            E_.measure("E.weight_in", (np.abs(Wnext - w_on) / w_in)[go & thin_ev])
        E_.require(~(dies | (is_vol & (w_after <= 0)))[go])                    # a path that ended has no further vertex
        pdf_dev = np.abs(pdf_dir / hg_pdf(c, gg) - 1)
        E_.measure("E.pdf", pdf_dev[sc & ~hard], count=False)
        if (sc & hard).any():
            # ... and there the HG value passes as everywhere else, or else in units of what ONE rounding (2^-53) of the
            # cosine does to it: d ln p / dc = 3 g / (1 + g^2 - 2 g c), 1.5e4 at g = 0.99 and 1.5e6 at g = 0.999 in the
            # forward peak.  (Either, as in C: off the peak one rounding of the cosine moves the value by 1e-16, while the
            # cosine the audit derives from two recorded directions is the sampled one to 1e-11 only -- a direction off unit
            # length by B.unit turns by that much more or less, the MCML update taking |u| = 1 -- and the value follows.)
            per_rounding = 3 * np.abs(gg) / (1 + gg * gg - 2 * gg * c) * LD(2) ** -53
            E_.measure("E.pdf_roundings", np.where(pdf_dev <= LD(tol["E.pdf"]), LD(0), pdf_dev / per_rounding)[sc & hard], count=False)
    E_.require((pdf_dir == 0)[is_vol & (w_after <= 0)])
    E_.extra.update(roulette_survived=int(survives.sum()), roulette_died=int(dies.sum()))

    # ---------------------------------------------------------------- H: emission
    H_ = chk["H"]
    pos, sdir = np.array(src["pos"], dtype=LD), np.array(src["dir"], dtype=LD)
    sdir = sdir / _norm(sdir)
    has0 = cnt >= 1
    spec = np.zeros(n, dtype=LD)               # specular reflectance taken from every photon on entry
    n_spec_terms = 0
    if quad:
        ex = np.array(list(src["extra"])[:6], dtype=LD)
        ea, eb = ex[:3], ex[3:]
        nn = sdir
        if abs(nn[0]) > abs(nn[1]):
            v2 = np.array([-nn[2], 0, nn[0]], dtype=LD) / np.sqrt(nn[0] ** 2 + nn[2] ** 2)
        else:
            v2 = np.array([0, nn[2], -nn[1]], dtype=LD) / np.sqrt(nn[1] ** 2 + nn[2] ** 2)
        v3 = _cross(nn, v2)
        q = U[:, 0, :]
        ox, oy = 2 * q[:, 2] - 1, 2 * q[:, 3] - 1
        with np.errstate(all="ignore"):
            wide = np.abs(ox) > np.abs(oy)
            r = np.where(wide, ox, oy)
            th = np.where(wide, PI / 4 * (oy / ox), PI / 2 - PI / 4 * (ox / oy))
        th = np.where((ox == 0) & (oy == 0), LD(0), th)
        dx, dy = r * np.cos(th), r * np.sin(th)
        dz = np.sqrt(np.maximum(1 - dx * dx - dy * dy, LD(0)))
        d_exp = dx[:, None] * v2 + dy[:, None] * v3 + dz[:, None] * nn
        p_exp = pos + q[:, 0:1] * ea + q[:, 1:2] * eb + PUSH * d_exp
        H_.measure("H.point", np.abs(P[:, 0] - p_exp).max(axis=-1)[has0])
        H_.measure("H.dir", np.abs(D[:, 0] - d_exp).max(axis=-1)[has0], count=False)
        H_.measure("H.weight", np.abs(Wt[:, 0] - 1)[has0], count=False)
        area = _norm(_cross(ea, eb))
        with np.errstate(all="ignore"):
            H_.measure("H.pdf", np.maximum(np.abs(v["pdf_pos"][:, 0].astype(LD) * area - 1),
                                           np.abs(pdf_dir[:, 0] * PI / np.abs(_dot(D[:, 0], nn)) - 1))[has0], count=False)
    else:
        d_exp, w_exp = sdir, LD(1)
        if layered:
            l0 = [k for k in range(nl) if zb[k] <= pos[2] < zb[k + 1]]
            assert l0, "the audit covers sources inside the slab"
            H_.require((med[:, 0] == l0[0])[has0])
            n_ab, n_0 = LD(layers.get("n_above", 1.0)), n_m[lm[0]]
            if pos[2] == zb[0] and sdir[2] > 0 and n_ab != n_0:
                s_i = np.sqrt(sdir[0] ** 2 + sdir[1] ** 2)
                r0 = fresnel_angle_form(s_i, sdir[2], n_ab, n_0)
                nr = n_ab / n_0
                d_exp = np.array([nr * sdir[0], nr * sdir[1], np.sqrt(1 - (nr * s_i) ** 2)], dtype=LD)      # Snell
                w_exp = 1 - r0
                spec[:] = r0
                n_spec_terms = n
                H_.extra["specular"] = float(r0)
        else:
            H_.require((med[:, 0] == int(src.get("start_medium", 0)))[has0])
        H_.measure("H.point", np.abs(P[:, 0] - pos).max(axis=-1)[has0])
        H_.measure("H.dir", np.abs(D[:, 0] - d_exp).max(axis=-1)[has0], count=False)
        H_.measure("H.weight", np.abs(Wt[:, 0] - w_exp)[has0], count=False)
        H_.measure("H.pdf", np.maximum(np.abs(v["pdf_pos"][:, 0] - 1.0), np.abs(v["pdf_dir"][:, 0] - 1.0))[has0], count=False)

    # ---------------------------------------------------------------- I: fates and totals
    L = np.clip(cnt - 1, 0, K - 1)
    rows = np.arange(n)
    lastm = np.zeros((n, K), bool); lastm[rows, L] = has0
    ended = gone | dies | (is_vol & (w_after <= 0))                            # the event ends the path
    I.require(~(ended & ~lastm & live))
    e_last = ended[rows, L] & has0
    step_L = step[rows, L]
    capped = has0 & ~e_last & (step_L == max_steps)
    ma = med_after[rows, L]
    mid_after = lm[np.clip(ma, 0, nl - 1)] if layered else np.clip(ma, 0, len(media) - 1)
    clear = has0 & ~e_last & ~capped & (mu_t[mid_after] == 0)                 # non-interacting with nothing ahead
    if layered:       # nothing ahead in a layer only for a path along it
        kl, dzl = kind[rows, L], D[rows, L, 2]
        I.require(~clear | (dzl == 0))
    I.declined += int(clear.sum()) if not layered else 0                       # (no mesh scene of the suite has a clear medium)
    I.require(~has0 | e_last | capped | clear)                                 # every path ends for a reason
    w_end = w_on[rows, L]
    steps_exp = int(np.where(has0, np.where(e_last | capped, step_L, step_L + 1), 0).sum())
    top = gone & (nxt < 0) if layered else np.zeros_like(gone)
    bottom = gone & ~top if layered else np.zeros_like(gone)
    gl = gone[rows, L] & has0
    terms = {k: [] for k in COUNTERS}
    terms["w_escaped_top"] = Wt[rows, L][gl & top[rows, L]]
    terms["w_escaped_bottom"] = Wt[rows, L][gl & bottom[rows, L]]
    terms["w_escaped_mesh"] = np.concatenate([Wt[rows, L][gl] if not layered else np.zeros(0, LD),
                                              w_end[clear] if not layered else np.zeros(0, LD)])
    terms["w_capped"] = np.concatenate([w_end[capped], w_end[clear] if layered else np.zeros(0, LD)])
    terms["w_roulette_net"] = np.concatenate([w_after[dies & live], -(factor - 1) * w_after[survives & live]])
    terms["w_specular"] = spec[:n_spec_terms]
    I.extra["fates"] = dict(top=int((gl & top[rows, L]).sum()), bottom=int((gl & bottom[rows, L]).sum()),
                            mesh=int(gl.sum()) if not layered else 0, roulette=int((dies[rows, L] & has0).sum()),
                            weight0=int(((is_vol & (w_after <= 0))[rows, L] & has0).sum()), capped=int(capped.sum()),
                            nothing_ahead=int(clear.sum()))

    # ---------------------------------------------------------------- J: deposits
    gr = scene["grid"]
    nx, ny, nz = (int(s) for s in gr["shape"])
    org, vox = np.array(gr["origin"], dtype=LD), np.array(gr["voxel"], dtype=LD)
    dep_w = (Wt * absorb[mid])[is_vol]                                         # weight the photon loses
    dep_q = (Wt * inv_mu_t[mid])[is_vol] if int(scene.get("quantity", 0)) == 1 else dep_w
    f = (P[is_vol] - org) / vox
    shape = np.array([nx, ny, nz])
    near_face = (np.abs(f - np.rint(f)) < FACE_BAND).any(axis=1)
    cell = np.floor(f).astype(np.int64)
    inside = ((cell >= 0) & (cell < shape)).all(axis=1)
    lo = np.zeros(nx * ny * nz, dtype=LD); hi_extra = np.zeros(nx * ny * nz, dtype=LD)
    m_lo = np.zeros(nx * ny * nz, np.int64); m_extra = np.zeros(nx * ny * nz, np.int64)
    sure = ~near_face
    flat = (cell[:, 2] * ny + cell[:, 1]) * nx + cell[:, 0]
    np.add.at(lo, flat[sure & inside], dep_q[sure & inside])
    np.add.at(m_lo, flat[sure & inside], 1)
    abs_lo, lost_lo = dep_w[sure & inside], dep_w[sure & ~inside]
    amb_w = dep_w[near_face]
    for k in np.flatnonzero(near_face):        # (few) a deposit on a face may count to either neighbour, or in / out
        opts = [sorted({int(np.floor(f[k, a] - FACE_BAND)), int(np.floor(f[k, a] + FACE_BAND))}) for a in range(3)]
        for cx, cy, cz in itertools.product(*opts):
            if 0 <= cx < nx and 0 <= cy < ny and 0 <= cz < nz:
                hi_extra[(cz * ny + cy) * nx + cx] += dep_q[k]
                m_extra[(cz * ny + cy) * nx + cx] += 1
    J.extra.update(deposits=int(is_vol.sum()), ambiguous=int(near_face.sum()), outside=int((sure & ~inside).sum()))
    got = np.asarray(grid).reshape(-1)
    if grid_kind == "u64fx":
        assert got.dtype == np.uint64
        got = got.astype(LD) * LD(2) ** -40
        bound_lo, bound_hi = m_lo * LD(2) ** -40, (m_lo + m_extra) * LD(2) ** -40          # +-1 unit per deposit
    else:
        got = got.astype(LD)
        # m non-negative terms, each rounded three times (1 / mu_t or mu_a / mu_t, the product, the sum): (m + 2) 2^-52
        bound_lo = (m_lo + 2) * LD(2) ** -52 * lo
        bound_hi = (m_lo + m_extra + 2) * LD(2) ** -52 * (lo + hi_extra)
    under, over = lo - got, got - (lo + hi_extra)
    with np.errstate(all="ignore"):
        ratio = np.maximum(np.where(under > 0, under / bound_lo, LD(0)), np.where(over > 0, over / bound_hi, LD(0)))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    J.measure("J.voxel", ratio)
    J.extra["voxels_hit"] = int((m_lo > 0).sum())

    terms["w_absorbed"], terms["w_lost_outside_grid"] = abs_lo, lost_lo
    I.require(np.array([int(counters["photons"]) == n, int(counters["steps"]) == steps_exp]))
    I.extra.update(steps=steps_exp, steps_counter=int(counters["steps"]))
    slack_amb = amb_w.sum() if amb_w.size else LD(0)
    for k in COUNTERS:
        x = np.asarray(terms[k], dtype=LD)
        tot, mag, m = x.sum() if x.size else LD(0), np.abs(x).sum() if x.size else LD(0), x.size
        # any-order double summation of m terms, each a product rounded a few times: (m + 4) 2^-52 sum |x|
        bound = (m + 4) * LD(2) ** -52 * mag
        diff = np.abs(LD(counters[k]) - tot)
        if k in ("w_absorbed", "w_lost_outside_grid") and amb_w.size:          # face deposits may fall on either side
            diff = np.maximum(diff - slack_amb, LD(0)); bound = bound + (amb_w.size + 4) * LD(2) ** -52 * slack_amb
        if k == "w_roulette_net":       # (media of albedo < 2^-10: each term is right to a rounding of the weight that came in)
            rl = (dies | survives) & live & thin_ev
            bound = bound + LD(2) ** -52 * (Wt * np.where(survives, factor - 1, LD(1)))[rl].sum()
        if bound == 0:
            I.require(np.array([diff == 0]))
        else:
            I.measure("I.sum", np.array([diff / bound]))
        I.extra.setdefault("totals", {})[k] = float(tot)
    I.n += n
    return {k: c.result() for k, c in chk.items()}
