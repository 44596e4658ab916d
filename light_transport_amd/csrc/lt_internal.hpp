// lt_internal.hpp -- layouts and launcher declarations shared by the host API (lt_api.cpp, g++) and the gfx950 kernel
// files (hipcc): lt_walk.hip, lt_query.hip, lt_render.hip (on the __device__ functions of lt_device.hpp) and lt_logtally.hip,
// lt_tallysum.hip, lt_tallystats.hip, lt_tallyconv.hip, lt_tallylabel.hip (with lt_walk.hip on lt_tally.hpp); DESIGN.md section 1.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lt.h"

namespace ltk {

// |g| below which the walk samples Henyey-Greenstein by hg_small_g (lt_device.hpp) instead of the quotient form, whose error
// grows as eps / (2 |g|): at 2^-6 the quotient form is 7.5e-6 (f32) / 1.1e-14 (f64) off, ten times its error at g = 0.3 .. 0.9,
// hg_small_g 6e-8 / 6e-17.  The host marks such a medium by inv_2g = 0, as it always has g = 0.
constexpr double kHgSmallG = 0.015625;

// Per-medium constants in walk precision R.  Derived values are computed on the
// host in double, one IEEE operation each, then narrowed.
template <typename R>
struct MedD {
    R mu_t, inv_mu_t, absorb, g;
    R n, one_m_g2, one_p_g2, inv_2g;   // inv_2g = 0 for |g| < kHgSmallG: the walk's test for hg_small_g
    R dep;   // what a voxel receives per unit of photon weight at an interaction: absorb, or inv_mu_t (LT_QUANTITY_FLUENCE)
    R one_m_g, two_g;   // the walk's Henyey-Greenstein denominator: (1 - g) + (2 g) xi as one fused product
    R pad_;
};

// Plane interface k of a layered slab (between layer k - 1 above and layer k below; k = 0 / n_layers: the ambient media):
// the refractive indices on both sides and their two quotients, computed once on the host (one IEEE division each, in walk
// precision) instead of by every photon that reaches the plane -- the Fresnel block of S/path_tracing_fix1.py:86-119
// runs whenever ANY lane of a wave sits on an interface, which in a layered medium is most wave-steps.
template <typename R>
struct IfD {
    R n_up, n_dn;        // index above / below the plane
    R nr_down, nr_up;    // n1 / n2 for a photon travelling down (n_up / n_dn) and up (n_dn / n_up)
};

// Everything a step of the slab walk reads about the layer it is in, as ONE record indexed by the layer: the medium's constants
// (copies of the MedD fields, bit for bit -- no layer -> medium indirection in front of the free path) and the layer's own two
// bounds (zb[l], zb[l + 1]).  Values that are used together share a 16-byte quad (pairs in f64, whole quads in f32), so a
// step fetches the record with six wide LDS reads (three in f32) instead of a dependent index read and seven narrow ones.
// Built on the host by fill_layer_records (lt_api.cpp) whenever the media or the layers change.
template <typename R>
struct alignas(16) LayD {
    R mu_t, inv_mu_t;        // free path
    R z_lo, z_hi;            // the layer's bounds: the step takes z_hi when uz > 0, z_lo otherwise
    R absorb, dep;           // drop
    R two_g, one_m_g;        // Henyey-Greenstein: denominator ...
    R one_m_g2, one_p_g2;    // ... numerator and offset ...
    R inv_2g, n;             // ... and scale (0: |g| < kHgSmallG, sampled from g = two_g / 2 alone); the refractive index (the interface table carries it for the slab's own events)
};
static_assert(sizeof(LayD<double>) == 96 && sizeof(LayD<float>) == 48, "LayD: a whole number of 16-byte quads");
// (host only, no device needed) the record of every layer from the media / bounds tables the kernels already get
template <typename R>
inline void fill_layer_records(const MedD<R>* media, const R* zb, const int32_t* layer_medium, int n_layers, LayD<R>* out)
{
    for (int l = 0; l < n_layers; l++) {
        const MedD<R>& m = media[layer_medium[l]];
        LayD<R>& r = out[l];
        r.mu_t = m.mu_t; r.inv_mu_t = m.inv_mu_t; r.z_lo = zb[l]; r.z_hi = zb[l + 1];
        r.absorb = m.absorb; r.dep = m.dep; r.two_g = m.two_g; r.one_m_g = m.one_m_g;
        r.one_m_g2 = m.one_m_g2; r.one_p_g2 = m.one_p_g2; r.inv_2g = m.inv_2g; r.n = m.n;
    }
}

// Triangle record: role of PreComputedTriangle (primitives.py:99-112).
template <typename R>
struct TriD {
    R a[3], ab[3], ac[3], n[3];
    int32_t med_front, med_back;
};

// kslack of the f32 plane pre-test (plane_within_reach, lt_device.hpp) for one triangle record: 16 roundings (8 float
// epsilons) times the conditioning |ab| |ac| / |ab x ac| of the triangle test at vertex a.  A zero-area triangle is never hit
// and asks for nothing.  A walk uses the largest value of its mesh (WalkParams::reach_slack).
static inline float reach_slack(const TriD<float>& T)
{
    const double ab[3] = {T.ab[0], T.ab[1], T.ab[2]}, ac[3] = {T.ac[0], T.ac[1], T.ac[2]};
    const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
    const double n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const double e2 = (ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2]) * (ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2]);
    if (!(n2 > 0) || !(e2 > 0)) return 0.0f;
    const double k = 8.0 * 1.1920928955078125e-07 * __builtin_sqrt(e2 / n2);
    return k < 1e30 ? (float)k : 1e30f;
}

// Flattened BVH node: role of LinearBVHNode (bvh_new.py:60-67).
template <typename R>
struct NodeD {
    R lo[3], hi[3];
    int32_t offset, n_prims, axis;
    int32_t skip;  // first node after this node's subtree (stackless traversal)
};

struct DevCounters {
    unsigned long long photons, steps;
    double w[8];  // absorbed, lost, esc_top, esc_bot, esc_mesh, specular, roulette, capped
};
enum { CW_ABSORBED = 0, CW_LOST, CW_ESC_TOP, CW_ESC_BOT, CW_ESC_MESH, CW_SPECULAR, CW_ROULETTE, CW_CAPPED };

constexpr int kMaxMedia = 32;
constexpr uint32_t kLogChunk = 8192;    // records per log chunk = records per partition work item
constexpr uint32_t kTileShift = 14;     // grid tile = 32 x 32 x 16 voxels = 16384 (128 KiB of f64 in LDS)
constexpr uint32_t kTileSize = 1u << kTileShift;
// Deposit records carry a TILED voxel index: (tile id << 14) | (z&15)<<10 | (y&31)<<5 | (x&31), tile id =
// (tz * nty + ty) * ntx + tx.  3-D blocks follow the compact photon cloud, so far fewer tiles are active than with
// slabs of consecutive linear indices and the partition pass writes longer contiguous runs.
constexpr uint32_t kTileBX = 5, kTileBY = 5, kTileBZ = 4;
// The first partition pass claims output space with one returning global atomic per (work item, non-empty digit).
// Records cluster in a few dozen tiles, so EVERY work item hits the same hot cursors, and one address sustains only
// ~90 atomics per microsecond (MI355X_MICROARCH "dequeue" / "fanin"); and a digit's region is written in fragments of
// tens of records, which only become whole 128-byte lines if neighbouring fragments meet in ONE XCD's L2.  Both are
// answered by groups: walk workgroup b belongs to group b % kLogGroups, takes its chunks from the group's own
// counter (chunk index = group + kLogGroups * n), and counts its records in the group's histogram column; partition
// workgroup b handles the chunks c = b (mod grid), i.e. one group's, and workgroups b and b + 8 share an XCD (observed
// dispatch order -- speed only, never correctness).  A digit's region is the groups' sub-regions back to back, each
// with its own cursor: 1/16 of the atomics per address, and consecutive fragments of a sub-region come from the same
// XCD shortly after one another.  Pass 2 of the two-pass form does the same with kLogGroups2 groups of work items.
constexpr uint32_t kLogGroups = 16;
constexpr uint32_t kLogGroups2 = 8;
constexpr int kMaxLayers = 64;

// March grid (meshes whose tables do not fit LDS, GEOM 2): a uniform grid over the root bounds of the BVH.  Every cell has
// an 8-byte record -- x: c0 (f32 bits, rounded down to a multiple of 64 ulp), a strictly conservative lower bound of the
// distance from ANY point of the cell to ANY triangle (a hop shorter than that cannot hit: no query at all), with the
// number of the cell's candidates in the 6 low bits; y: where they start in `list` -- and the candidates are every
// triangle that overlaps the cell grown by a margin (exact triangle / box separating-axis test on the host).  A query marches its hop segment through the
// cells front to back (3-D DDA; free space is crossed c0 at a time) and tests the candidates of the cells it visits with the
// walk's own tri_hit: same predicate, same nearest / tie rule, hence the same answer as a brute-force scan -- without a
// per-lane pointer chase through a tree.  Role of intersect_bvh's near-child-first order (S/bvh_new.py:455-458).
constexpr uint32_t kMarchCountMask = 63u;       // low bits of a cell record's x word: candidates of the cell (63: more than 62 -> that query walks the BVH)
struct MarchGrid {
    const uint2* cell;          // [nz][ny][nx]
    const uint32_t* list;
    int nx, ny, nz;
    double org[3], inv[3], h[3];   // origin, 1 / cell size, cell size
    // the dimensions as reals and everything again in f32: a kernel reads its loop invariants in walk precision straight
    // from its arguments (scalar registers) -- converted inside the kernel they are vector registers held through the hot loop
    double fn[3];
    float org32[3], inv32[3], h32[3], fn32[3];
    double nudge64, nudge32;       // by how much the f64 / f32 march steps past a cell wall (<< the margin of the lists)
};

// A photon in flight, as walk_kernel<..., PHASE 1> hands it over and walk_kernel<..., PHASE 2> takes it up (see "tail split"
// in lt_walk_kernel.inc): everything the walk keeps per lane -- position, direction, weight, unused optical depth, layer,
// step count, id, and the XORWOW state (rocrand_state_xorwow without the Box-Muller cache: d + x[5]).
template <typename R>
struct SurvD {
    R p[3], u[3], w, sleft;
    unsigned long long pid;
    int32_t cur;
    uint32_t step;
    uint32_t rng[6];
    uint32_t held[3];        // mesh walks: the decision uniforms of a prepared step that waits for its surface query (HeldU bits)
    uint32_t q_pend;         //             ... and whether there is one
};
constexpr uint32_t kDumpMaxLanes = 32;     // a wave hands its photons over when the queue is empty and at most this many are alive (default)
constexpr uint32_t kDumpPoolLanes = 48;    // what the pool is sized for per wave (the knob tail_split = n sets the threshold, at most this)

struct WalkParams {
    // photon queue
    unsigned long long* head;
    unsigned long long n_photons, photon_offset, seed;
    // scene tables (device pointers, element type depends on walk precision)
    const void* media;
    const void* zb;
    const void* ifaces;         // IfD<R>[n_layers + 1]
    const void* layers;         // LayD<R>[n_layers]: the slab walk's per-layer step records
    const int32_t* layer_medium;
    const void* tris;
    const void* nodes;
    const int16_t* links;       // [8][2][n_nodes] front-to-back threading of the BVH (bvh_octant_links); null beyond 32767 nodes
    int n_media, n_layers, n_tris, n_nodes;
    double n_above, n_below;
    // voxel grid
    void* grid;
    int nx, ny, nz, tally;
    double origin[3], inv_voxel[3];
    double fdim[3];       // (double)nx, ny, nz -- and below everything the hot loop compares positions with, again in f32: read in
                          // walk precision from the kernel arguments these are scalar operands; an int -> real or f64 -> f32
                          // conversion inside the kernel is hoisted in front of the loop and kept in a vector register
    double cdim[3];       // clearance grid dimensions as reals
    struct { float origin[3], inv_voxel[3], fdim[3], corg[3], cinv[3], cdim[3]; } f32;
    // source
    int src_type, start_medium;
    double src_pos[3], src_dir[3], src_e1[3], src_e2[3];
    // table RNG
    const double* table;
    unsigned long long table_steps;
    unsigned max_steps;
    unsigned query_min;   // mesh walks: lanes of a wave that wait for a surface query before it is served (0: the built-in default)
    DevCounters* counters;
    // log-structured tally (null = deposit with global atomics): coalesced deposit log written by the walk,
    // reduced into the grid by the partition / tile-reduce kernels
    uint32_t* log_idx;    // [log_cap_chunks * kLogChunk] voxel index
    void* log_val;        // [log_cap_chunks * kLogChunk] value in the tally's type
    uint32_t* log_fill;   // [log_cap_chunks] valid records per chunk (zeroed per batch: chunk indices are claimed per group)
    uint32_t* log_next;   // [kLogGroups] chunks claimed per group; chunk index = group + kLogGroups * n
    uint32_t log_cap_chunks;
    uint32_t* log_hist;   // [log_n_hist][kLogGroups] records per partition bin and group, accumulated by the walk (LDS histogram per workgroup):
                          // bin = tile id >> (log_hist_shift - kTileShift): the tile itself for grids of <= 1024 tiles,
                          // the level-1 digit of the two-pass partition otherwise (<= 128 bins: 512 B of LDS)
    uint32_t log_n_hist, log_hist_shift, log_ntx, log_nty;
    uint32_t* log_overflow;   // [1] records that found the log full and went to the grid as global atomics
    // clearance grid (mesh scenes; null = off), one 16-byte record per cell:
    //   x  c0 (f32 bits): conservative lower bound of the distance from any point of the cell to any triangle -- a hop
    //      shorter than that cannot hit, so no query is made at all;
    //   y  c2 | c4 << 16 (f16, rounded down): the same bound for the 3rd / the 5th nearest triangle -- a hop shorter
    //      than c2 (c4) can only hit the 2 (4) nearest ones, which are tested directly instead of walking the BVH;
    //   z  id0 | id1 << 16,  w  id2 | id3 << 16: those triangles, nearest first (0xffff: none)
    const uint4* clear;
    int cnx, cny, cnz;
    double corg[3], cinv[3];
    MarchGrid mg;         // GEOM 2 (cell == null: off -> every hop walks the BVH)
    // tail split (slab walks in log mode): pool of photons handed from the bulk kernel to the tail kernel
    void* pool;           // SurvD<R>[pool_cap]
    uint32_t* pool_n;     // entries claimed (may exceed pool_cap: the excess was not written and those photons walked on)
    uint32_t pool_cap;
    uint32_t dump_max;    // PHASE 1: hand over when at most this many lanes of the wave are alive
    // light sub-path capture (null = off)
    lt_vertex* vertices;
    uint32_t* vertex_counts;
    unsigned max_vertices;
    float reach_slack;    // f32 mesh walks in LDS: kslack of plane_within_reach, the largest reach_slack() of the mesh's triangles
                          // (it sits in what was the struct's tail padding: no other member moves)
};

struct LaunchCfg {
    int blocks, threads;
    size_t lds_bytes;
};

#define LT_TALLY_NONE 3  /* beside lt.h's LT_TALLY_*: diagnostic build of the walk without deposition (not part of the ABI) */
// walk variants: precision x geometry x rng are compile-time, tally is too
struct Variant {
    int f32;     // 0: f64 walk, 1: f32 walk
    int mesh;    // 0: layered slab, 1: mesh + BVH staged in LDS, 2: mesh + BVH read from global memory, 3: the same with a march grid (walk_kernel_m)
    int table;   // 0: XORWOW, 1: table RNG
    int tally;   // LT_TALLY_* or LT_TALLY_NONE
    int capture; // 1: the build that stores light sub-path vertices (f64 walk, XORWOW)
    int phase;   // slab walks: 0 whole walk, 1 bulk (hands the last photons of every wave to a pool), 2 tail (walks the pool)
    int route;   // slab walks: kRouteAtomic / kRouteLog, a build each.  launch_walk sets it from WalkParams::log_idx, whatever it is
                 // given; a caller sets it for walk_max_blocks_per_cu alone.  (The mesh walks test log_idx themselves.)
};
constexpr int kRouteAtomic = 0;   // deposit records go to the grid as global atomics
constexpr int kRouteLog = 1;      // ... into the deposit log

hipError_t launch_walk(const WalkParams& P, const Variant& v, const LaunchCfg& cfg, hipStream_t s);
size_t walk_lds_bytes(const Variant& v, int n_media, int n_layers, int n_tris, int n_nodes, unsigned n_hist = 0);
// resident-blocks-per-CU the runtime reports for a variant at `threads`
int walk_max_blocks_per_cu(const Variant& v, int threads, size_t lds_bytes);

struct RenderParams {
    const void* tris;    // TriD<double>
    const void* nodes;   // NodeD<double>
    const lt_surface_material* mats;
    const lt_point_light* lights;
    const int16_t* links;   // [8][2][n_nodes] front-to-back threading of the BVH per direction sign pattern (nearest_bvh_render);
                            // null beyond 32767 nodes: the BVH is then searched in storage order
    int n_tris, n_nodes, n_lights;
    int W, H, S, D;
    double cam[3], f_distance;
    const double* xs;
    const double* ys;
    double* rand_0;
    const double* rand_1;
    const int32_t* light_choice;
    double* image;
    int variant;   // 0 = path_tracing_fix1.trace_path, 1 = path_tracing_old.trace_path
    int choices;   // variant 1: light_choice entries per sample
    int lds_tables;   // variant 0: 0 = scene tables always in global memory (lt_set_tuning "render_lds_tables"), else in LDS where they fit
};
constexpr int kRenderOldMaxDepth = 24;   // frames of the unrolled recursion (variant 1)
// march grid: exact point-to-mesh distance per cell by a pruned BVH nearest-point query, seeded from a coarse pass
// (`coarse`: scratch of ceil(n/8)^3 doubles); fills the x word of every cell record
hipError_t launch_march_clearance(const void* tris_f64, const void* nodes_f64, int n_nodes, const MarchGrid& G, uint2* cells,
                                  double* coarse, hipStream_t s);
hipError_t launch_build_clearance(const void* tris_f64, int n_tris, int near_lists, void* clear_records, int nx, int ny, int nz,
                                  const double org[3], const double cell[3], hipStream_t s);
hipError_t launch_render_surface(const RenderParams& P, hipStream_t s);

// Per-batch bookkeeping words of the log pipeline (one u32 array per lane, zeroed before every batch).
enum { LM_NEXT = 0,        // [kLogGroups] chunks the walk claimed per group (may run past the capacity when the log overflowed)
       LM_OVERFLOW = 16,   // records that went to the grid as atomics because the log was full
       LM_RECORDS,         // totals: records in the log
       LM_ITEMS2,          //         pass-2 work items (4096-record slices; statistics only)
       LM_ITEMS_R,         //         reduce work items
       LM_SLICE,           //         records per reduce work item (chosen by the scan from the record count)
       LM_ITEMS_C,         //         pass-2 work units = k_log_count2 work items (two-pass form)
       LM_WORK,            // work-item counter of the reduce (the other passes stride the grid over equal-sized items)
       LM_WORDS = 24 };
static_assert(kLogGroups == 16, "LM_NEXT holds one counter per group");
// tile / bin regions start at multiples of these record counts so that the wide (16-byte) loads of the next pass are
// aligned; the gaps are never read (a region's length comes from the histogram), the buffers carry the slack
constexpr uint32_t kTileAlign = 8, kBinAlign = 8;     // (a hot tile's bin is read by the reduce: 8 records per 16-byte load)

// log-structured tally pipeline (all on stream s)
struct LogReduceParams {
    const uint32_t* log_idx; const void* log_val; const uint32_t* log_fill;   // walk output
    uint32_t* tmp_idx; void* tmp_val;          // ping-pong buffers, same capacity as the log
    uint32_t* hist1;                           // [nb1][kLogGroups] records per level-1 bin and group (two-pass form: the walk's histogram)
    uint32_t* hist;                            // records per tile: one-pass form [n_tiles][kLogGroups], the walk's histogram;
                                               //                   two-pass form [n_tiles][kLogGroups2], counted from pass 1's output
    uint32_t* bin_base; uint32_t* bin_cnt;     // [nb1 + 1] / [nb1] where pass 1 puts each level-1 bin, records in it
    uint32_t* tile_base; uint32_t* tile_cnt;   // [n_tiles + 1] / [n_tiles] where the final pass puts each tile, records in it
    uint32_t* cursor1;                         // [nb1][kLogGroups] (one-pass form: [n_tiles][kLogGroups])
    uint32_t* cursor2;                         // [n_tiles][kLogGroups2]
    uint32_t* items2;                          // [nb1 + 1] prefix of pass-2 work items per level-1 bin
    uint32_t* items_c;                         // [nb1 + 1] prefix of tile-count work items per level-1 bin
    uint32_t* itab;                            // [pass-2 units][4] descriptor of every pass-2 work unit (k_log_items2)
    uint32_t* items_r;                         // [n_tiles + 1] prefix of reduce work items per tile
    uint32_t* meta;                            // [LM_WORDS]
    unsigned long long* job;                   // [2] records / overflowed records of the whole launch (all batches)
    uint32_t cap_chunks;
    uint32_t n_tiles, bits2;                   // level-2 digit width; level-1 bins = ceil(n_tiles >> bits2); 0 = one pass
    void* grid; size_t n_vox; int tally;
    uint32_t nx, ny, nz, ntx, nty;             // grid shape and tile counts along x, y (tiled record index)
    // Hot-tile form of the two-pass partition (null / 0: off).  dmap[tile] = digit of pass 1: the H tiles that held the
    // most records when the map was made ("hot", H = dmeta[0]) have digits 0 .. H-1 of their own and leave pass 1 in
    // their final form; every other tile shares digit H + (tile >> bits2) with its level-1 bin and goes through pass 2.
    // Any map gives the same grid; a good one (k_log_plan, from a measured tile histogram) saves the second pass for
    // most records.  The walk's level-1 histogram is not used in this form: k_log_count1 counts the digits from the log.
    const uint16_t* dmap; const uint32_t* dmeta;
    int alone;                                 // nothing shares the device with this lane's reduction (one lane, walk at full occupancy):
                                               // the partition may take the register budget that leaves no room for a co-running walk
    int flush_atomic;                          // every tile adds to the grid with atomics (another lane of the same
                                               // launch may be updating it at the same time)
};
hipError_t launch_log_scan_bins(const LogReduceParams& L, hipStream_t s);
hipError_t launch_log_count1(const LogReduceParams& L, hipStream_t s);      // hot-tile form: pass-1 digit histogram from the log
// hot-tile map from a tile histogram: at most max_hot tiles, the ones with the most records (dmeta[0] = their number)
hipError_t launch_log_plan(const uint32_t* tile_cnt, uint32_t n_tiles, uint32_t bits2, uint32_t max_hot, uint16_t* dmap,
                           uint32_t* dmeta, hipStream_t s);
uint32_t log_max_digits();  // digits one partition pass can tell apart (1024)
constexpr uint32_t kMaxHotTiles = 8192;    // the map lives in LDS (2 bytes per tile: 16 KiB beside a partition item's 56 KiB, two workgroups per CU)
hipError_t launch_log_scan_tiles(const LogReduceParams& L, hipStream_t s);
hipError_t launch_log_part1(const LogReduceParams& L, hipStream_t s);
hipError_t launch_log_part2(const LogReduceParams& L, hipStream_t s);
hipError_t launch_log_reduce(const LogReduceParams& L, hipStream_t s);
uint32_t log_part_item();   // records per partition work item (the log capacity is a multiple of it)

// use_bvh: 0 brute force, 1 BVH, 2 / 3 march grid (G; falls back to the BVH for origins outside the grid), 4 BVH front to back (links)
hipError_t launch_intersect_rays(const void* tris, const void* nodes, int n_tris, int n_nodes,
                                 const double* o, const double* d, const double* tmax, size_t n,
                                 int use_bvh, const MarchGrid* G, const int16_t* links, int32_t* prim, double* t, hipStream_t s);
hipError_t launch_triangle_intersect(const double* o, const double* d, const double* tris, size_t n,
                                     double* t, hipStream_t s);
hipError_t launch_intersect_bounds(const double* o, const double* d, const double* tmax,
                                   const double* boxes, size_t n, int32_t* hit, hipStream_t s);
hipError_t launch_eval(int fn, const double* in, size_t n, double* out, hipStream_t s);
hipError_t launch_rng_raw(unsigned long long seed, unsigned long long photon_id, unsigned count,
                          uint32_t* out, hipStream_t s);
hipError_t launch_grid_to_f64(const void* grid, int tally, size_t n, double* out, hipStream_t s);
hipError_t launch_grid_add(void* dst, const void* src, int tally, size_t n, hipStream_t s);   // dst += src

// Sums of the voxel tally on the device (lt_tallysum.hip).  The *_plan functions (host only) say what a call needs: the sums
// go through partial sums in a scratch buffer of `partial_bytes`; out gets n_out doubles, raw (null unless the tally is u64
// fixed point) the integer sums.  keep_mask 0..6 (bit 0 x, 1 y, 2 z); bins: device copy of the [ny][nx] table, every entry
// checked by the caller to lie in -1 .. n_bins - 1 (the kernel indexes LDS with it).
size_t tally_sum_axes_plan(int nx, int ny, int nz, int keep_mask, int tally, size_t* partial_bytes);   // returns n_out
hipError_t launch_tally_sum_axes(const void* grid, int tally, int nx, int ny, int nz, int keep_mask, void* partials, double* out,
                                 unsigned long long* raw, hipStream_t s);
constexpr int kMaxSumBins = 4096;    // the bins of a column sum live in LDS, 8 bytes each
size_t tally_sum_columns_plan(int nx, int ny, int nz, int n_bins);   // returns partial_bytes; n_out = nz * n_bins
hipError_t launch_tally_sum_columns(const void* grid, int tally, int nx, int ny, int nz, const int32_t* bins, int n_bins, void* partials,
                                    double* out, unsigned long long* raw, hipStream_t s);
// the finishing pass of those sums on its own: out[i] = partial[0][i] + ... + partial[P - 1][i] in a fixed order; partial
// [P][n_out] u64 (integer != 0: out = sum * 2^-40, raw -- may be null -- the sum) or f64 (raw is not used)
hipError_t launch_tally_sum_finish(const void* partial, int integer, uint32_t P, size_t n_out, double* out, unsigned long long* raw,
                                   hipStream_t s);

// Statistical error of the tally from batch moments (lt_tallystats.hip).  prev: the grid at the last fold, in the tally's type;
// m2: f64 per voxel.  The summary goes through stats_summary_parts(...) x (n_edges + 2) x 16 bytes of partial sums and leaves
// in `out`, n_edges + 2 8-byte words each: the weight per class (f64), the raw weight (u64 fixed point only), the voxels (u64),
// and one more block that is not used.  edges: host array, checked by the caller (finite, >= 0, ascending, 1 .. kMaxStatEdges).
constexpr int kMaxStatEdges = 63;
hipError_t launch_stats_fold(const void* grid, void* prev, double* m2, int tally, size_t n, hipStream_t s);
hipError_t launch_stats_relerr(const void* prev, const double* m2, int tally, size_t n, uint64_t batches, double* out, hipStream_t s);
uint32_t stats_summary_parts(size_t n_vox, int tally);
hipError_t launch_stats_summary(const void* prev, const double* m2, int tally, size_t n, uint64_t batches, const double* edges,
                                int n_edges, void* partials, double* out, hipStream_t s);

// The tally convolved in x and y (lt_tallyconv.hip).  All tap pointers are device copies, checked by the caller (finite, >= 0,
// odd counts within the limits).  The tile kernel takes its taps FLIPPED in both axes, every row of kw taps zero-padded to
// conv_padded(kw): ft [kh][conv_padded(kw)]; the separable form ftx [conv_padded(kw)] and fty [kh] (flipped, not padded), with
// `mid` an intermediate of out's size.  grid: the whole tally; planes z0 .. z0 + nz_out - 1 are convolved into out
// [nz_out][ny][nx].  The _at form takes taps [kh][kw] as the caller gave them and cols [n_cols][2] = (ix, iy) inside the grid;
// out [nz][n_cols].
constexpr int kMaxConvTaps = 63, kMaxConvTapsSep = 255, kMaxConvColumns = 4096;
constexpr int kConvPad = 4;
constexpr int conv_padded(int kw) { return (kw + kConvPad - 1) / kConvPad * kConvPad; }
size_t tally_conv_lds_bytes(int kh, int kw);    // LDS of one workgroup of the tile kernel (kw = 0: the column pass of the separable form)
hipError_t launch_tally_convolve(const void* grid, int tally, int nx, int ny, int z0, int nz_out, const double* ft, int kh, int kw,
                                 double* out, hipStream_t s);
hipError_t launch_tally_convolve_sep(const void* grid, int tally, int nx, int ny, int z0, int nz_out, const double* ftx, int kw,
                                     const double* fty, int kh, double* mid, double* out, hipStream_t s);
hipError_t launch_tally_convolve_at(const void* grid, int tally, int nx, int ny, int nz, const double* taps, int kh, int kw,
                                    const int32_t* cols, int n_cols, double* out, hipStream_t s);

// A box of the tally, binned (lt_tallybox.hip).  lo, size, bin in x, y, z order, checked by the caller: lo >= 0, size and bin
// >= 1, the box inside the nx x ny x nz grid.  out [oz][oy][ox] doubles with o = ceil(size / bin); raw (null unless the tally
// is u64 fixed point) the integer sums.  No partial sums: nothing but out and raw is written.
hipError_t launch_tally_box(const void* grid, int tally, int nx, int ny, const int32_t lo[3], const int32_t size[3], const int32_t bin[3],
                            double* out, unsigned long long* raw, hipStream_t s);

// The tally by region (lt_tallylabel.hip): every voxel booked under (label, class of its own value).  labels: device copy of
// the label volume, one byte per voxel (0 .. n_labels - 1; anything else: left out), or null = label 0 everywhere.  edges: host
// array, checked by the caller as for the statistics; n_edges 0 .. kMaxStatEdges (0: one class).  partials:
// tally_label_partial_bytes(...); out: tally_label_out_bytes(...), 8-byte words with bins = n_labels * (n_edges + 1): weight f64
// [bins], raw weight u64 [bins] (u64 fixed point only), NON-ZERO voxels u64 [bins], zero voxels u64 [n_labels] and, with
// want_peak, the bits of the largest element u64 [n_labels] (a float's in the low bits) and the lowest flat index that holds it
// u32 [n_labels] -- 0xffffffff for a label whose peak is 0: the caller knows its first voxel.
constexpr int kMaxLabels = 64;
uint32_t tally_label_parts(size_t n_vox, int tally);
size_t tally_label_partial_bytes(size_t n_vox, int tally, int n_labels, int n_edges);
size_t tally_label_out_bytes(int n_labels, int n_edges);
hipError_t launch_tally_label_bins(const void* grid, const uint8_t* labels, int tally, size_t n, int n_labels, const double* edges,
                                   int n_edges, int want_peak, void* partials, double* out, hipStream_t s);

// The tally along rays (lt_tallyrays.hip).  Rays and camera are checked by the caller (finite, d != 0, 0 <= t_lo < t_hi); every
// pointer is a device pointer.  o, d [n][3], t_range [n][2] or null = [0, +inf); xs [width], ys [height].  An output that is null is
// not written; the kernel instantiated is the one for tally_ray_mask(out) (1 integral, 2 maximum, 4 first crossing; 1, 2, 4 and 7
// exist, any other combination takes 7).
struct TallyRayGrid { int n[3]; double origin[3], voxel[3]; };      // x, y, z order
struct TallyRayOut { double* integral; double* max_w; int64_t* max_index; double* first_t; int64_t* first_index; };
int tally_ray_mask(const TallyRayOut& out);
hipError_t launch_tally_rays(const void* grid, int tally, const TallyRayGrid& g, const double* o, const double* d, const double* t_range,
                             size_t n, double threshold, const TallyRayOut& out, hipStream_t s);
hipError_t launch_tally_view(const void* grid, int tally, const TallyRayGrid& g, int width, int height, const double camera[3],
                             double f_distance, const double* xs, const double* ys, double threshold, const TallyRayOut& out, hipStream_t s);

}  // namespace ltk
