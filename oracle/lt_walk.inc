/*
 * lt_walk.inc -- precision-generic body of the CPU oracle (TEST INFRASTRUCTURE
 * ONLY, see lt_oracle.h).  Included twice by lt_oracle.c with
 *   R      real type            SFX(name)  name suffixed _f64 / _f32
 *   RLOG RSIN RCOS RSQRT RFABS RFMA  libm functions of that precision
 * Reference citations use S/ = LightTransportSimulator/light_transport/src/.
 */

#define R_EPSILON ((R)1e-6) /* S/constants.py:12 */
#define R_TRI_EPS ((R)1e-7) /* S/intersects.py:56 */
#define R_INF ((R)INFINITY)

/* ---- small vector helpers ------------------------------------------------ */
static inline R SFX(dot3)(const R* a, const R* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static inline void SFX(cross3)(const R* a, const R* b, R* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
static inline void SFX(normalize3)(R* v) /* S/vectors.py:6-7 */
{
    R l = RSQRT(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] /= l; v[1] /= l; v[2] /= l;
}

/* ---- triangle record: role of PreComputedTriangle (S/primitives.py:99-112) - */
typedef struct SFX(tri) {
    R a[3];  /* vertex_1 */
    R ab[3]; /* edge_1 = vertex_2 - vertex_1 */
    R ac[3]; /* edge_2 = vertex_3 - vertex_1 */
    R n[3];  /* normalize(cross(edge_1, edge_2)) */
    int32_t med_front, med_back;
} SFX(tri);

/* Moller-Trumbore, restating triangle_intersect (S/intersects.py:46-104).
 * Returns t, or NaN where the reference returns None. */
static inline R SFX(tri_hit)(const R* o, const R* d, const SFX(tri)* T)
{
    R ddn = SFX(dot3)(d, T->n);
    if (RFABS(ddn) <= R_TRI_EPS) return (R)NAN;            /* :69-72 */
    R pvec[3], qvec[3], tvec[3];
    SFX(cross3)(d, T->ac, pvec);                           /* :74 */
    R det = SFX(dot3)(T->ab, pvec);                        /* :77 */
    if (-R_TRI_EPS < det && det < R_TRI_EPS) return (R)NAN; /* :79 */
    R inv_det = (R)1 / det;
    tvec[0] = o[0] - T->a[0]; tvec[1] = o[1] - T->a[1]; tvec[2] = o[2] - T->a[2];
    R u = SFX(dot3)(tvec, pvec) * inv_det;                 /* :86 */
    if (u < 0 || u > 1) return (R)NAN;
    SFX(cross3)(tvec, T->ab, qvec);                        /* :91 */
    R v = SFX(dot3)(d, qvec) * inv_det;                    /* :94 */
    if (v < 0 || u + v > 1) return (R)NAN;
    R t = SFX(dot3)(T->ac, qvec) * inv_det;                /* :99 */
    return (t > R_TRI_EPS) ? t : (R)NAN;                   /* :101-104 */
}

/* gamma(3) with float32 machine epsilon (S/intersects.py:229-235) */
static inline R SFX(gamma3)(void)
{
    const R eps = (R)5.9604644775390625e-08; /* np.finfo(float32).eps * 0.5 */
    return ((R)3 * eps) / ((R)1 - (R)3 * eps);
}

/* slab test restating intersect_bounds (S/intersects.py:179-196): t0 = 0,
 * t1 = tmax, far side widened by 1 + 2*gamma(3). */
static inline int SFX(box_hit)(const R* lo, const R* hi, const R* o, const R* inv_d, R tmax)
{
    R t0 = 0, t1 = tmax;
    const R widen = (R)1 + (R)2 * SFX(gamma3)();
    for (int i = 0; i < 3; i++) {
        R tn = (lo[i] - o[i]) * inv_d[i];
        R tf = (hi[i] - o[i]) * inv_d[i];
        if (tn > tf) { R s = tn; tn = tf; tf = s; }
        tf *= widen;
        t0 = tn > t0 ? tn : t0;
        t1 = tf < t1 ? tf : t1;
        if (t0 > t1) return 0;
    }
    return 1;
}

typedef struct SFX(node) {
    R lo[3], hi[3];
    int32_t offset, n_prims, axis;
} SFX(node);

/* Nearest hit with the reference predicate EPSILON < t < min_distance
 * (S/bvh_new.py:438; min_distance starts at ray.tmax, :420).  Ties in t go to
 * the lower primitive index, which is what a brute-force scan in index order
 * with the strict '<' returns -- the parity target (SURVEY.md B3: the
 * reference traversal itself mis-skips nodes and is NOT reproduced). */
static inline void SFX(consider)(const SFX(tri)* tris, int i, const R* o, const R* d,
                                 int* best_i, R* best_t)
{
    R t = SFX(tri_hit)(o, d, &tris[i]);
    if (t == t && t > R_EPSILON) {
        if (t < *best_t || (t == *best_t && *best_i >= 0 && i < *best_i)) { *best_t = t; *best_i = i; }
    }
}

static void SFX(nearest_brute)(const SFX(tri)* tris, int n_tris, const R* o, const R* d,
                               R tmax, int* prim, R* t_out)
{
    int bi = -1; R bt = tmax;
    for (int i = 0; i < n_tris; i++) SFX(consider)(tris, i, o, d, &bi, &bt);
    *prim = bi; *t_out = bi >= 0 ? bt : R_INF;
}

static void SFX(nearest_bvh)(const SFX(tri)* tris, const SFX(node)* nodes, int n_nodes,
                             const R* o, const R* d, R tmax, int* prim, R* t_out)
{
    int bi = -1; R bt = tmax;
    if (n_nodes > 0) {
        R inv_d[3] = {(R)1 / d[0], (R)1 / d[1], (R)1 / d[2]}; /* S/bvh_new.py:418 */
        int neg[3] = {inv_d[0] < 0, inv_d[1] < 0, inv_d[2] < 0};
        const R slack = (R)1 + (R)2 * SFX(gamma3)();
        /* one pending sibling per level: the stack grows with the tree's depth, which the library does not limit (its
         * device traversal is stackless) -- 64 entries inline, the heap beyond that */
        int small[64]; int* stack = small; int cap = 64, sp = 0, cur = 0;
        for (;;) {
            const SFX(node)* nd = &nodes[cur];
            if (SFX(box_hit)(nd->lo, nd->hi, o, inv_d, bt * slack)) {
                if (nd->n_prims > 0) {
                    for (int k = 0; k < nd->n_prims; k++)
                        SFX(consider)(tris, nd->offset + k, o, d, &bi, &bt);
                    if (sp == 0) break;
                    cur = stack[--sp];
                } else {
                    if (sp == cap) {
                        int* bigger = (int*)malloc((size_t)cap * 2 * sizeof(int));
                        memcpy(bigger, stack, (size_t)cap * sizeof(int));
                        if (stack != small) free(stack);
                        stack = bigger; cap *= 2;
                    }
                    if (neg[nd->axis]) { /* S/bvh_new.py:455-458: far child first */
                        stack[sp++] = cur + 1; cur = nd->offset;
                    } else {
                        stack[sp++] = nd->offset; cur = cur + 1;
                    }
                }
            } else {
                if (sp == 0) break;
                cur = stack[--sp];
            }
        }
        if (stack != small) free(stack);
    }
    *prim = bi; *t_out = bi >= 0 ? bt : R_INF;
}

/* ---- sampling ------------------------------------------------------------- */
/* henyey_greenstein value, S/medium_samples.py:14-16 (pbrt sign convention) */
static inline R SFX(hg_pdf)(R cos_t, R g)
{
    R denom = (R)1 + g * g + (R)2 * g * cos_t;
    return (R)0.07957747154594767 * ((R)1 - g * g) / (denom * RSQRT(denom));
}

/* HG inverse CDF in the deflection-angle convention (SURVEY.md App. C.6);
 * pdf(cos) = henyey_greenstein(-cos, g). */
static inline R SFX(hg_sample)(R xi, R g)
{
    R c;
    if (g == 0) c = (R)2 * xi - (R)1;
    else {
        R t = ((R)1 - g * g) / ((R)1 - g + (R)2 * g * xi);
        c = ((R)1 + g * g - t * t) * ((R)1 / ((R)2 * g));
    }
    if (c > 1) c = 1;
    if (c < -1) c = -1;
    return c;
}

/* ... as the WALK samples it.  The quotient form above cancels as g -> 0: ((1 + g^2) - t^2) / (2 g) is wrong by eps / (2 |g|),
 * by 1e-10 at g = 1e-6 in double, and in float every scattering is at exactly 90 degrees from |g| = 1e-8 down.  Below
 * R_HG_SMALL_G (the library's kHgSmallG) the walk takes the same law written as the isotropic answer plus a correction of
 * order g, in which nothing cancels; at g = 0 it is 2 xi - 1 to the bit. */
#define R_HG_SMALL_G ((R)0.015625)
/* the medium's g in walk precision: a |g| < 1 that rounds to 1 in float (1 - g = 0) goes to the largest float below 1 */
static inline R SFX(narrow_g)(double g)
{
    R r = (R)g;
    if (fabs(g) < 1.0 && !(fabs((double)r) < 1.0)) r = RNEXT(r, (R)0);
    return r;
}
static inline R SFX(hg_sample_walk)(R xi, R g)
{
    if (!(RFABS(g) < R_HG_SMALL_G)) return SFX(hg_sample)(xi, g);
    /* (the fused multiply-adds of the library's hg_small_g, written out there as here) */
    const R s = RFMA((R)2, xi, (R)-1);
    const R d = RFMA(g, s, (R)1);
    const R a = RFMA(-s, s, (R)1);
    const R b = RFMA(g, RFMA((R)2, s, -g), (R)3);
    R c = s + ((g * a) * b) / ((R)2 * (d * d));
    if (c > 1) c = 1;
    if (c < -1) c = -1;
    return c;
}

/* create_orthonormal_system, S/utils.py:72-80 */
static inline void SFX(onb)(const R* n, R* v2, R* v3)
{
    if (RFABS(n[0]) > RFABS(n[1])) {
        R l = RSQRT(n[0] * n[0] + n[2] * n[2]);
        v2[0] = -n[2] / l; v2[1] = 0; v2[2] = n[0] / l;
    } else {
        R l = RSQRT(n[1] * n[1] + n[2] * n[2]);
        v2[0] = 0; v2[1] = n[2] / l; v2[2] = -n[1] / l;
    }
    SFX(cross3)(n, v2, v3);
}

/* concentric_sample_disk, S/utils.py:115-128 */
static inline void SFX(disk)(R u0, R u1, R* d)
{
    R ox = (R)2 * u0 - (R)1, oy = (R)2 * u1 - (R)1;
    if (ox == 0 && oy == 0) { d[0] = 0; d[1] = 0; return; }
    R r, theta;
    if (RFABS(ox) > RFABS(oy)) { r = ox; theta = (R)0.7853981633974483 * (oy / ox); }
    else { r = oy; theta = (R)1.5707963267948966 - (R)0.7853981633974483 * (ox / oy); }
    d[0] = r * RCOS(theta); d[1] = r * RSIN(theta);
}

/* cosine_weighted_hemisphere_sampling, S/utils.py:132-161.
 * out[0..2] = direction, out[3] = pdf. */
static inline void SFX(cosine_hemi)(const R* n, const R* wi_in, R u0, R u1, R* out)
{
    R wi[3] = {-wi_in[0], -wi_in[1], -wi_in[2]};      /* :133 */
    R d[2]; SFX(disk)(u0, u1, d);
    R zz = (R)1 - d[0] * d[0] - d[1] * d[1];
    R z = RSQRT(zz > 0 ? zz : 0);                      /* :138 */
    R oz = z;
    R v2[3], v3[3]; SFX(onb)(n, v2, v3);
    if (wi[2] < 0) oz = -oz;                           /* :145-146 */
    R pdf = (wi[2] * oz > 0) ? RFABS(z) * (R)0.3183098861837907 : 0; /* :149-152 */
    for (int k = 0; k < 3; k++) out[k] = d[0] * v2[k] + d[1] * v3[k] + oz * n[k]; /* :154-157 */
    out[3] = pdf;
}

/* The walk's emission, role of cosine_weighted_light_sampling (S/light_samples.py:64-85): a cosine lobe about the source
 * normal n, whatever way n points -- an emitter has no incoming direction, and cosine_hemi's mirror test (:145-146, meant for
 * the z of a direction in the surface's own frame) sent the photons of a source with n.z < 0 into the hemisphere behind it.
 * Same disk map and frame as cosine_hemi. */
static inline void SFX(cosine_lobe)(const R* n, R u0, R u1, R* out)
{
    R d[2]; SFX(disk)(u0, u1, d);
    R zz = (R)1 - d[0] * d[0] - d[1] * d[1];
    R z = RSQRT(zz > 0 ? zz : 0);
    R v2[3], v3[3]; SFX(onb)(n, v2, v3);
    for (int k = 0; k < 3; k++) out[k] = d[0] * v2[k] + d[1] * v3[k] + z * n[k];
    out[3] = z * (R)0.3183098861837907;
}

/* get_reflected_direction, S/brdf.py:8-9 */
static inline void SFX(reflect)(const R* v, const R* n, R* o)
{
    R k = (R)2 * SFX(dot3)(v, n);
    o[0] = v[0] - k * n[0]; o[1] = v[1] - k * n[1]; o[2] = v[2] - k * n[2];
    SFX(normalize3)(o);
}

/* Dielectric boundary (SURVEY.md App. C.5).  d = unit travel direction,
 * nf = unit normal FACING the incoming photon (d.nf <= 0).  Returns the exact
 * unpolarised Fresnel reflectance; *cos_t and refr[] are set when R < 1.
 * Refraction vector form follows S/path_tracing_fix1.py:107-114 with
 * Nr = n1/n2; total internal reflection when the radicand <= 0 (:110). */
static inline R SFX(boundary)(const R* d, const R* nf, R n1, R n2, R* cos_t_out, R* refr)
{
    R cos_i = -SFX(dot3)(d, nf);
    if (n1 == n2) {
        *cos_t_out = cos_i; refr[0] = d[0]; refr[1] = d[1]; refr[2] = d[2];
        return 0;
    }
    R Nr = n1 / n2;
    R rad = (R)1 - Nr * Nr * ((R)1 - cos_i * cos_i);
    if (rad <= 0) { *cos_t_out = 0; refr[0] = refr[1] = refr[2] = 0; return 1; }
    R cos_t = RSQRT(rad);
    R a = n1 * cos_i, b = n2 * cos_t, c = n1 * cos_t, e = n2 * cos_i;
    R rs = (a - b) / (a + b), rp = (c - e) / (c + e);
    R k = Nr * cos_i - cos_t;
    refr[0] = d[0] * Nr + nf[0] * k;
    refr[1] = d[1] * Nr + nf[1] * k;
    refr[2] = d[2] * Nr + nf[2] * k;
    SFX(normalize3)(refr);
    *cos_t_out = cos_t;
    return (R)0.5 * (rs * rs + rp * rp);
}

/* The same event at a PLANE z = const (layered slabs), where it specialises exactly: cos_i = |uz|; the reflected direction is
 * (ux, uy, -uz) -- v - 2 (v.n) n with n = (0, 0, +-1) without any rounding -- and the refracted one (Nr ux, Nr uy,
 * sign(uz) cos_t), of unit length by Snell's law (Nr^2 (1 - uz^2) + cos_t^2 = 1): neither is renormalised.  Returns the
 * unpolarised Fresnel reflectance, 1 for total internal reflection (radicand <= 0, S/path_tracing_fix1.py:110). */
static inline R SFX(boundary_planar)(R uz, R n1, R n2, R Nr, R* cos_t_out)
{
    R cos_i = RFABS(uz);
    if (n1 == n2) { *cos_t_out = cos_i; return 0; }
    R rad = (R)1 - Nr * Nr * ((R)1 - cos_i * cos_i);
    if (rad <= 0) { *cos_t_out = 0; return 1; }
    R cos_t = RSQRT(rad);
    R a = n1 * cos_i, b = n2 * cos_t, c = n1 * cos_t, e = n2 * cos_i;
    R rs = (a - b) / (a + b), rp = (c - e) / (c + e);
    *cos_t_out = cos_t;
    return (R)0.5 * (rs * rs + rp * rp);
}

/* Spin: rotate unit direction u by deflection cosine ct and azimuth 2*pi*xi
 * (standard MCML update with the |uz| > 0.99999 special case, App. C.6). */
static inline void SFX(spin)(R* u, R ct, R xi_phi)
{
    R st2 = (R)1 - ct * ct;
    R st = RSQRT(st2 > 0 ? st2 : 0);
    R phi = (R)6.283185307179586 * xi_phi;
    R cp = RCOS(phi), sp = RSIN(phi);
    R ux = u[0], uy = u[1], uz = u[2];
    if (RFABS(uz) > (R)0.99999) {
        u[0] = st * cp; u[1] = st * sp; u[2] = uz >= 0 ? ct : -ct;
    } else {
        R t2 = (R)1 - uz * uz;
        R tmp = RSQRT(t2);
        u[0] = st * (ux * uz * cp - uy * sp) / tmp + ux * ct;
        u[1] = st * (uy * uz * cp + ux * sp) / tmp + uy * ct;
        u[2] = -st * cp * tmp + uz * ct;
    }
}

/* ---- the walk (SURVEY.md Appendix C; PARITY UNPINNED vs the reference) ---- */
typedef struct SFX(med) {
    R mu_t, inv_mu_t, absorb, g, n;
    R dep;   /* what a voxel receives per unit of photon weight at an interaction: absorb (LT_QUANTITY_ABSORBED) or
                1 / mu_t = absorb / mu_a (LT_QUANTITY_FLUENCE: fluence x voxel volume, defined for mu_a = 0 too) */
} SFX(med);

typedef struct SFX(world) {
    const lto_scene* sc;
    SFX(med)* med;
    R* zb;               /* layer bounds in R */
    SFX(tri)* tris;
    SFX(node)* nodes;
    R origin[3], inv_voxel[3];
    R src_pos[3], src_dir[3], src_e1[3], src_e2[3];
    const double* table; uint64_t table_steps; uint64_t photon_offset; uint64_t seed;
    uint32_t max_steps;
    double* grid_f64; uint64_t* grid_fx; int atomic_grid;
    lt_vertex* vertices; uint32_t* vcounts; unsigned max_vertices; /* f4 capture, NULL = off */
} SFX(world);

typedef struct SFX(acc) {
    uint64_t steps;
    double absorbed, lost, esc_top, esc_bot, esc_mesh, specular, roulette, capped;
} SFX(acc);

/* dw: weight the photon loses here (energy bookkeeping); dq: what the voxel receives (the tally quantity) */
static inline void SFX(deposit)(const SFX(world)* W, SFX(acc)* A, const R* p, R dw, R dq)
{
    const lto_scene* sc = W->sc;
    R fx = (p[0] - W->origin[0]) * W->inv_voxel[0];
    R fy = (p[1] - W->origin[1]) * W->inv_voxel[1];
    R fz = (p[2] - W->origin[2]) * W->inv_voxel[2];
    if (fx >= 0 && fx < (R)sc->nx && fy >= 0 && fy < (R)sc->ny && fz >= 0 && fz < (R)sc->nz) {
        size_t idx = ((size_t)(int)fz * (size_t)sc->ny + (size_t)(int)fy) * (size_t)sc->nx + (size_t)(int)fx;
        A->absorbed += (double)dw;
        if (W->grid_f64) {
            if (W->atomic_grid) lto_atomic_add_f64(&W->grid_f64[idx], (double)dq);
            else W->grid_f64[idx] += (double)dq;
        }
        if (W->grid_fx) {
            uint64_t q = (uint64_t)((double)dq * LT_FX_SCALE + 0.5);
            if (W->atomic_grid) __atomic_fetch_add(&W->grid_fx[idx], q, __ATOMIC_RELAXED);
            else W->grid_fx[idx] += q;
        }
    } else {
        A->lost += (double)dw;
    }
}

static inline void SFX(record)(const SFX(world)* W, uint64_t rel, unsigned* nv, const R* p, const R* u, R w,
                               int kind, int medium, unsigned step, const R* gn, R pdf_pos, R pdf_dir)
{
    if (W->vertices && *nv < W->max_vertices) {
        lt_vertex* v = W->vertices + rel * (uint64_t)W->max_vertices + *nv;
        for (int k = 0; k < 3; k++) { v->point[k] = (double)p[k]; v->direction[k] = (double)u[k]; v->g_norm[k] = gn ? (double)gn[k] : 0.0; }
        v->throughput = (double)w; v->pdf_pos = (double)pdf_pos; v->pdf_dir = (double)pdf_dir;
        v->kind = kind; v->medium = medium; v->step = step; v->pad_ = 0;
        (*nv)++;
        W->vcounts[rel] = *nv;
    }
}

/* uniforms of group `grp` of photon `pid`, all in (0,1] */
static inline void SFX(uniforms)(const SFX(world)* W, lto_xorwow* rng, uint64_t pid, uint64_t grp, R* u)
{
    if (W->table) { /* table RNG: S/scene.py:68-69, S/path_tracing_fix1.py:28-29 */
        const double* t = W->table + ((pid - W->photon_offset) * W->table_steps + grp) * 4;
        for (int k = 0; k < 4; k++) u[k] = (R)(1.0 - t[k]);
    } else {
        for (int k = 0; k < 4; k++) u[k] = SFX(lto_uniform32)(rng);  /* xi0..xi3: one 32-bit draw each (4 per group) */
    }
}

static void SFX(walk_one)(const SFX(world)* W, SFX(acc)* A, uint64_t pid)
{
    const lto_scene* sc = W->sc;
    lto_xorwow rng; lto_photon_stream(&rng, W->seed, pid);
    uint64_t grp = 0;
    R u4[4];
    R p[3], u[3], w = 1, sleft = 0;
    int cur; /* layer index (layers) or medium id (mesh) */
    const int layered = sc->n_layers > 0;

    /* ---- emission: role of sample_light, S/light_samples.py:90-116 ---- */
    R e_pdf_pos = 1, e_pdf_dir = 1; /* light vertex (S/light_samples.py:83,100); a pencil beam is a delta source */
    if (sc->src_type == LT_SRC_COSINE_QUAD) {
        SFX(uniforms)(W, &rng, pid, grp++, u4);
        R o4[4];
        SFX(cosine_lobe)(W->src_dir, u4[2], u4[3], o4);
        e_pdf_dir = RFABS(o4[0] * W->src_dir[0] + o4[1] * W->src_dir[1] + o4[2] * W->src_dir[2]) * (R)0.3183098861837907; /* |cos| / pi, S/light_samples.py:83 */
        { R cr[3]; SFX(cross3)(W->src_e1, W->src_e2, cr); e_pdf_pos = (R)1 / RSQRT(SFX(dot3)(cr, cr)); }
        for (int k = 0; k < 3; k++) {
            u[k] = o4[k];
            p[k] = W->src_pos[k] + u4[0] * W->src_e1[k] + u4[1] * W->src_e2[k] + R_EPSILON * o4[k]; /* :96 */
        }
    } else {
        for (int k = 0; k < 3; k++) { p[k] = W->src_pos[k]; u[k] = W->src_dir[k]; }
    }
    if (layered) {
        cur = -1;
        for (int l = 0; l < sc->n_layers; l++)
            if (p[2] >= W->zb[l] && p[2] < W->zb[l + 1]) { cur = l; break; }
        if (cur < 0) { A->esc_top += (double)w; return; } /* launched outside the slab */
        if (sc->src_type == LT_SRC_PENCIL && p[2] == W->zb[0] && u[2] > 0) {
            /* specular reflection on entering the first layer */
            R n2 = W->med[sc->layer_medium[0]].n, n1 = (R)sc->n_above;
            if (n1 != n2) {
                R nf[3] = {0, 0, -1}, ct, refr[3];
                R Rs = SFX(boundary)(u, nf, n1, n2, &ct, refr);
                A->specular += (double)(w * Rs);
                w -= w * Rs;
                if (!(w > 0)) return;
                u[0] = refr[0]; u[1] = refr[1]; u[2] = refr[2];
            }
        }
    } else {
        cur = sc->start_medium;
    }

    unsigned nv = 0;
    const uint64_t rel = pid - W->photon_offset;
    if (W->vertices) W->vcounts[rel] = 0;
    SFX(record)(W, rel, &nv, p, u, w, LT_VERTEX_LIGHT, cur, 0u, W->src_dir, e_pdf_pos, e_pdf_dir);

    uint64_t max_steps = W->max_steps;
    if (W->table) {
        uint64_t cap = W->table_steps > grp ? W->table_steps - grp : 0;
        if (cap < max_steps) max_steps = cap;
    }

    for (uint64_t step = 0;; step++) {
        if (step >= max_steps) { A->capped += (double)w; return; }
        SFX(uniforms)(W, &rng, pid, grp++, u4);
        A->steps++;
        const SFX(med)* M = &W->med[layered ? sc->layer_medium[cur] : cur];
        if (sleft == 0) sleft = -RLOG(u4[0]);
        R s = (M->mu_t > 0) ? sleft * M->inv_mu_t : R_INF;

        /* ---- hop: distance to the next boundary ---- */
        R tb = R_INF; int hit_tri = -1;
        if (layered) {
            if (u[2] > 0) tb = (W->zb[cur + 1] - p[2]) / u[2];
            else if (u[2] < 0) tb = (W->zb[cur] - p[2]) / u[2];
        } else {
            R th;
            SFX(nearest_bvh)(W->tris, W->nodes, sc->n_nodes, p, u, s, &hit_tri, &th);
            if (hit_tri >= 0) tb = th;
        }
        int at_boundary = layered ? (tb <= s) : (hit_tri >= 0);
        if (!at_boundary && !(s < R_INF)) { /* non-interacting and nothing ahead */
            if (layered) A->capped += (double)w; else A->esc_mesh += (double)w;
            return;
        }

        if (at_boundary) {
            p[0] += u[0] * tb; p[1] += u[1] * tb; p[2] += u[2] * tb;
            sleft -= tb * M->mu_t;
            if (!(sleft > 0)) sleft = 0;
            if (layered) {
                /* plane interface: boundary_planar; n1 / n2 rounded once, as the library's interface table holds it */
                const int down = u[2] > 0;
                const int next = down ? cur + 1 : cur - 1;
                p[2] = down ? W->zb[cur + 1] : W->zb[cur];
                R n1 = M->n, n2;
                if (next < 0) n2 = (R)sc->n_above;
                else if (next >= sc->n_layers) n2 = (R)sc->n_below;
                else n2 = W->med[sc->layer_medium[next]].n;
                const R Nr = n1 / n2;
                R ct;
                const R Rf = SFX(boundary_planar)(u[2], n1, n2, Nr, &ct);
                const int refl = u4[3] <= Rf;
                const int gone = !refl && (next < 0 || next >= sc->n_layers);
                {   /* a delta event: pdf_dir = probability of the branch taken (0: the photon leaves the scene) */
                    const R nf[3] = {0, 0, down ? (R)-1 : (R)1};
                    SFX(record)(W, rel, &nv, p, u, w, refl ? LT_VERTEX_REFLECTIVE : LT_VERTEX_TRANSMISSIVE, cur, (unsigned)(step + 1), nf,
                                (R)0, gone ? (R)0 : (refl ? Rf : (R)1 - Rf));
                }
                if (refl) u[2] = -u[2];                        /* S/brdf.py:8-9 at a plane */
                else if (gone) {
                    if (next < 0) A->esc_top += (double)w; else A->esc_bot += (double)w;
                    return;
                } else { u[0] *= Nr; u[1] *= Nr; u[2] = down ? ct : -ct; cur = next; }   /* S/path_tracing_fix1.py:107-114 at a plane */
                continue;
            }
            R nf[3], n1 = M->n, n2; int next;
            {
                const SFX(tri)* T = &W->tris[hit_tri];
                R dn = SFX(dot3)(u, T->n);
                R sg = dn > 0 ? (R)-1 : (R)1;            /* S/path_tracing_fix1.py:48-51 */
                nf[0] = sg * T->n[0]; nf[1] = sg * T->n[1]; nf[2] = sg * T->n[2];
                next = dn > 0 ? T->med_front : T->med_back;
                n2 = next >= 0 ? W->med[next].n : n1; /* exterior: index matched */
            }
            R ct, refr[3];
            R Rf = SFX(boundary)(u, nf, n1, n2, &ct, refr);
            {   /* a delta event: pdf_dir = probability of the branch taken (0: the photon leaves the scene) */
                const int refl = u4[3] <= Rf;
                const int leaves = !refl && next < 0;
                SFX(record)(W, rel, &nv, p, u, w, refl ? LT_VERTEX_REFLECTIVE : LT_VERTEX_TRANSMISSIVE, cur, (unsigned)(step + 1), nf,
                            (R)0, leaves ? (R)0 : (refl ? Rf : (R)1 - Rf));
            }
            if (u4[3] <= Rf) { /* reflect: S/brdf.py:8-9 */
                R ro[3]; SFX(reflect)(u, nf, ro);
                u[0] = ro[0]; u[1] = ro[1]; u[2] = ro[2];
                for (int k = 0; k < 3; k++) p[k] += R_EPSILON * nf[k]; /* :118 */
            } else {
                if (next < 0) { A->esc_mesh += (double)w; return; }
                u[0] = refr[0]; u[1] = refr[1]; u[2] = refr[2];
                for (int k = 0; k < 3; k++) p[k] -= R_EPSILON * nf[k]; /* :112 */
                cur = next;
            }
            continue;
        }

        /* ---- interaction site: move, drop, spin, roulette ---- */
        p[0] += u[0] * s; p[1] += u[1] * s; p[2] += u[2] * s;
        sleft = 0;
        R dw = w * M->absorb;
        const R ct_s = g_plant_cos0 ? (R)0 : SFX(hg_sample_walk)(u4[1], M->g);
        SFX(record)(W, rel, &nv, p, u, w, LT_VERTEX_VOLUME, cur, (unsigned)(step + 1), NULL, (R)0,
                    (w - dw > 0) ? SFX(hg_pdf)(-ct_s, M->g) : (R)0);
        SFX(deposit)(W, A, p, dw, w * M->dep);
        w -= dw;
        if (!(w > 0)) return;
        SFX(spin)(u, ct_s, u4[2]);
        if (w < (R)1e-4) { /* weight roulette, shape of S/path_tracing_fix1.py:126-132 */
            if (u4[3] <= (R)0.1) { A->roulette -= 9.0 * (double)w; w *= (R)10; }
            else { A->roulette += (double)w; return; }
        }
    }
}

typedef struct SFX(job) {
    const SFX(world)* W; uint64_t lo, hi; SFX(acc) A;
} SFX(job);

static void* SFX(job_main)(void* arg)
{
    SFX(job)* J = (SFX(job)*)arg;
    memset(&J->A, 0, sizeof J->A);
    for (uint64_t i = J->lo; i < J->hi; i++) SFX(walk_one)(J->W, &J->A, i);
    return NULL;
}

static int SFX(prepare)(SFX(world)* W, const lto_scene* sc)
{
    memset(W, 0, sizeof *W);
    W->sc = sc;
    W->med = (SFX(med)*)calloc((size_t)sc->n_media + 1, sizeof(SFX(med)));
    for (int i = 0; i < sc->n_media; i++) {
        double mu_t = sc->media[i].mu_a + sc->media[i].mu_s;
        W->med[i].mu_t = (R)mu_t;
        W->med[i].inv_mu_t = (R)(mu_t > 0 ? 1.0 / mu_t : 0.0);
        W->med[i].absorb = (R)(mu_t > 0 ? sc->media[i].mu_a / mu_t : 0.0);
        W->med[i].dep = sc->quantity == LT_QUANTITY_FLUENCE ? W->med[i].inv_mu_t : W->med[i].absorb;
        W->med[i].g = SFX(narrow_g)(sc->media[i].g);
        W->med[i].n = (R)sc->media[i].n;
    }
    if (sc->n_layers > 0) {
        W->zb = (R*)calloc((size_t)sc->n_layers + 1, sizeof(R));
        for (int i = 0; i <= sc->n_layers; i++) W->zb[i] = (R)sc->z_bounds[i];
    }
    if (sc->n_tris > 0) {
        W->tris = (SFX(tri)*)calloc((size_t)sc->n_tris, sizeof(SFX(tri)));
        for (int i = 0; i < sc->n_tris; i++) {
            double f[16];
            lto_triangle_fields(sc->verts + (size_t)i * 9, 1, f);
            for (int k = 0; k < 3; k++) {
                W->tris[i].a[k] = (R)sc->verts[(size_t)i * 9 + k];
                W->tris[i].ab[k] = (R)f[3 + k];
                W->tris[i].ac[k] = (R)f[6 + k];
                W->tris[i].n[k] = (R)f[9 + k];
            }
            W->tris[i].med_front = sc->med_front ? sc->med_front[i] : -1;
            W->tris[i].med_back = sc->med_back ? sc->med_back[i] : -1;
        }
        W->nodes = (SFX(node)*)calloc((size_t)sc->n_nodes + 1, sizeof(SFX(node)));
        for (int i = 0; i < sc->n_nodes; i++) {
            for (int k = 0; k < 3; k++) {
                /* round outward so the box stays conservative in reduced precision */
                R lo = (R)sc->nodes[i].lo[k], hi = (R)sc->nodes[i].hi[k];
                if ((double)lo > sc->nodes[i].lo[k]) lo = RNEXT(lo, -R_INF);
                if ((double)hi < sc->nodes[i].hi[k]) hi = RNEXT(hi, R_INF);
                W->nodes[i].lo[k] = lo; W->nodes[i].hi[k] = hi;
            }
            W->nodes[i].offset = sc->nodes[i].offset;
            W->nodes[i].n_prims = sc->nodes[i].n_prims;
            W->nodes[i].axis = sc->nodes[i].axis;
        }
    }
    for (int k = 0; k < 3; k++) {
        W->origin[k] = (R)sc->origin[k];
        W->inv_voxel[k] = (R)(1.0 / sc->voxel[k]);
        W->src_pos[k] = (R)sc->src_pos[k];
        W->src_dir[k] = (R)sc->src_dir[k];
        W->src_e1[k] = (R)sc->src_extra[k];
        W->src_e2[k] = (R)sc->src_extra[3 + k];
    }
    W->max_steps = sc->max_steps;
    return 0;
}

static void SFX(release)(SFX(world)* W)
{
    free(W->med); free(W->zb); free(W->tris); free(W->nodes);
}

static int SFX(run)(const lto_scene* sc, uint64_t n_photons, uint64_t photon_offset,
                    uint64_t seed, const double* rng_table, uint64_t table_steps,
                    double* grid_f64, uint64_t* grid_fx, lt_counters* C, int n_threads,
                    lt_vertex* vertices, uint32_t* vcounts, unsigned max_vertices)
{
    SFX(world) W;
    SFX(prepare)(&W, sc);
    W.vertices = vertices; W.vcounts = vcounts; W.max_vertices = max_vertices;
    W.table = rng_table; W.table_steps = table_steps;
    W.photon_offset = photon_offset; W.seed = seed;
    W.grid_f64 = grid_f64; W.grid_fx = grid_fx;
    if (n_threads < 1) n_threads = 1;
    if ((uint64_t)n_threads > n_photons) n_threads = n_photons ? (int)n_photons : 1;
    W.atomic_grid = n_threads > 1;
    SFX(job)* jobs = (SFX(job)*)calloc((size_t)n_threads, sizeof(SFX(job)));
    pthread_t* th = (pthread_t*)calloc((size_t)n_threads, sizeof(pthread_t));
    for (int t = 0; t < n_threads; t++) {
        jobs[t].W = &W;
        jobs[t].lo = photon_offset + n_photons * (uint64_t)t / (uint64_t)n_threads;
        jobs[t].hi = photon_offset + n_photons * (uint64_t)(t + 1) / (uint64_t)n_threads;
    }
    if (n_threads == 1) SFX(job_main)(&jobs[0]);
    else {
        for (int t = 0; t < n_threads; t++) pthread_create(&th[t], NULL, SFX(job_main), &jobs[t]);
        for (int t = 0; t < n_threads; t++) pthread_join(th[t], NULL);
    }
    for (int t = 0; t < n_threads; t++) {
        C->steps += jobs[t].A.steps;
        C->w_absorbed += jobs[t].A.absorbed;
        C->w_lost_outside_grid += jobs[t].A.lost;
        C->w_escaped_top += jobs[t].A.esc_top;
        C->w_escaped_bottom += jobs[t].A.esc_bot;
        C->w_escaped_mesh += jobs[t].A.esc_mesh;
        C->w_specular += jobs[t].A.specular;
        C->w_roulette_net += jobs[t].A.roulette;
        C->w_capped += jobs[t].A.capped;
    }
    C->photons += n_photons;
    free(jobs); free(th);
    SFX(release)(&W);
    return 0;
}

#undef R_HG_SMALL_G
#undef R_EPSILON
#undef R_TRI_EPS
#undef R_INF
