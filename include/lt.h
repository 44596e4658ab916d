/*
 * lt.h -- C ABI of the MI355X photon-transport hot path (liblt_hip.so).
 *
 * The reference (zhouyifan233/light-transport) has no FFI: its only boundary is
 * the Python call  render_scene(scene, primitives, bvh) -> ndarray
 * (LightTransportSimulator/light_transport/src/path_tracing_fix1.py:139-169),
 * fed by constructor objects (primitives.py:99, material.py:28, scene.py:53,
 * bvh_new.py:11,60,148,282).  This header is the boundary a maintainer binds
 * with ctypes from the (empty) reference slot src/photon_tracing.py; see
 * INTEGRATION.md for the binding stub.  Each entry point names the reference
 * construct whose role it takes over.
 *
 * Conventions
 *   - every function returns 0 on success, a negative LT_E_* code on failure;
 *     lt_last_error(ctx) returns a message for the last failure on that ctx
 *     (ctx == NULL: the last failure of lt_create on this thread).
 *   - all host pointers stay owned by the caller; set_* functions copy.
 *   - one ctx = one GPU + one HIP stream.  A ctx is not thread-safe; distinct
 *     ctxs are independent.
 *   - there is NO CPU fallback: lt_create fails when no gfx950-class device /
 *     code object is usable.
 */
#ifndef LT_H_
#define LT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_ABI_VERSION 3

/* error codes */
#define LT_OK 0
#define LT_E_INVALID (-1)  /* bad argument / inconsistent scene            */
#define LT_E_STATE (-2)    /* call order: e.g. launch before set_grid      */
#define LT_E_HIP (-3)      /* HIP runtime error (message has the detail)   */
#define LT_E_NOMEM (-4)
#define LT_E_UNSUPPORTED (-5)

/* tally storage of the voxel grid (lt_set_grid) */
#define LT_TALLY_F32 0   /* global_atomic_add_f32                         */
#define LT_TALLY_F64 1   /* global_atomic_add_f64                         */
#define LT_TALLY_U64FX 2 /* u64 fixed point, 2^40 units per unit weight:
                            order-independent, bit-reproducible.  One voxel
                            holds at most 2^24 = 1.68e7 units of weight
                            before it wraps (C2's hottest voxel absorbs
                            0.0074 per photon: ~2e9 photons per grid);
                            read the grid out and zero it before that      */
#define LT_FX_SCALE 1099511627776.0 /* 2^40 */

/* what an interaction adds to its voxel (lt_set_tally_quantity) */
#define LT_QUANTITY_ABSORBED 0 /* the absorbed weight dw = w mu_a / mu_t (default)           */
#define LT_QUANTITY_FLUENCE 1  /* w / mu_t (= dw / mu_a, defined for mu_a = 0 too): the grid then holds
                                  fluence x voxel volume x photons, correct in heterogeneous media -- no division
                                  by a per-voxel mu_a afterwards.  Role of the normalised tally image / samples,
                                  path_tracing_fix1.py:162-166.  Counters keep booking the absorbed weight.    */

/* photon sources (lt_set_source) */
#define LT_SRC_PENCIL 0      /* pos, dir                                   */
#define LT_SRC_COSINE_QUAD 1 /* quad corner=pos, normal=dir,
                                extra[0..2]=edge1, extra[3..5]=edge2;
                                cosine-weighted about dir (reference
                                utils.py:132-161, light_samples.py:64-116) */

/* lt_launch flags */
#define LT_FLAG_F32_WALK 1u /* walk arithmetic in f32 (default: f64, the
                               reference's dtype, e.g. scene.py:31-50)     */

/* optical medium -- takes the role of Material.ior (material.py:22) plus the
 * volumetric coefficients the reference lacks. */
typedef struct lt_medium {
    double mu_a; /* absorption coefficient  [1/length] */
    double mu_s; /* scattering coefficient  [1/length] */
    double g;    /* Henyey-Greenstein anisotropy (medium_samples.py:14-16), any
                    |g| < 1: sampled without cancellation down to g = 0; a g
                    that rounds to +-1 in an f32 walk is taken as the largest
                    float below 1.  The deflection cosine is good to a few
                    roundings of the walk's precision for |g| <= 0.9 and loses
                    a factor ~ 1 / (1 - |g|)^2 of it towards |g| = 1 */
    double n;    /* refractive index */
} lt_medium;

/* flattened BVH node, DFS pre-order -- role of LinearBVHNode
 * (bvh_new.py:60-67) with second_child_offset = FIRST index of the right
 * subtree (the reference's own "#TODO: fix this", bvh_new.py:295). */
typedef struct lt_bvh_node {
    double lo[3];
    double hi[3];
    int32_t offset;  /* leaf: primitives_offset; interior: second child   */
    int32_t n_prims; /* >0: leaf                                           */
    int32_t axis;    /* interior: split axis 0..2                          */
    int32_t pad_;
} lt_bvh_node;

/* energy bookkeeping.  Invariant:
 *   photons = w_absorbed + w_lost_outside_grid + w_escaped_top
 *           + w_escaped_bottom + w_escaped_mesh + w_specular
 *           + w_roulette_net + w_capped                                  */
typedef struct lt_counters {
    uint64_t photons;
    uint64_t steps; /* photon-steps: iterations of the hop/drop/spin loop */
    double w_absorbed;
    double w_lost_outside_grid;
    double w_escaped_top;
    double w_escaped_bottom;
    double w_escaped_mesh;
    double w_specular;
    double w_roulette_net;
    double w_capped;
} lt_counters;

typedef struct lt_ctx lt_ctx;

/* ---- lifetime ---------------------------------------------------------- */
int lt_abi_version(void);
/* role of: constructing a Scene (scene.py:53-73) bound to one device */
int lt_create(lt_ctx** out, int device_id);
int lt_destroy(lt_ctx* ctx);
const char* lt_last_error(const lt_ctx* ctx);

/* ---- scene ------------------------------------------------------------- */
/* media table; index = medium id used by layers / triangles */
int lt_set_media(lt_ctx* ctx, const lt_medium* media, int n);
/* layered slab: n layers, z_bounds[n+1] ascending (last may be +inf),
 * ambient indices above z_bounds[0] / below z_bounds[n].  Clears any mesh. */
int lt_set_layers(lt_ctx* ctx, const double* z_bounds, const int32_t* medium_idx,
                  int n, double n_above, double n_below);
/* triangle mesh + flattened BVH.  verts [T][3][3] (role of
 * PreComputedTriangle.vertex_1..3, primitives.py:99-111, in BVH order =
 * ordered_prims of build_bvh, bvh_new.py:148).  med_front/med_back: medium id
 * on the +normal / -normal side, -1 = exterior (photon leaves the scene).
 * Clears any layers. */
int lt_set_mesh(lt_ctx* ctx, const double* verts, const int32_t* med_front,
                const int32_t* med_back, int n_tris, const lt_bvh_node* nodes,
                int n_nodes);
/* Host BVH build + flatten in one call -- role of build_bvh + flatten_bvh (bvh_new.py:148-300) over BoundedBox-es of the
 * triangles (bvh_new.py:11-15), with the reference's defects B1 (second_child_offset) and B2 (partition on a copy) fixed.
 * Pure host code: no ctx, no device.  verts [n_tris][3][3]; split_method 1 = midpoint (the reference's hard-wired choice,
 * :149), 0 = binned surface-area heuristic (its dormant branch, :198-258).  order_out [n_tris]: ordered_prims[i] is input
 * triangle order_out[i]; nodes_out [max_nodes >= 2 n_tris - 1], pre-order, as lt_set_mesh takes them.  The tree equals
 * the Python mirror's (light_transport_amd/src/bvh_new.py build_bvh / flatten_bvh) node for node. */
int lt_build_bvh(const double* verts, int n_tris, int split_method, int32_t* order_out, lt_bvh_node* nodes_out,
                 int max_nodes, int* n_nodes_out);
/* The tables a layered slab hands its walk kernels, built on the host exactly as lt_launch builds them.  Pure host code: no ctx,
 * no device.  f32 != 0: walk precision float (every output then holds floats), else double.  media_out [n_media][12]: the
 * per-medium record (mu_t, 1/mu_t, absorb, g, n, 1-g^2, 1+g^2, 1/(2g), dep, 1-g, 2g, 0); zb_out [n_layers + 1]: the bounds in
 * walk precision; rec_out [n_layers][12]: the per-layer step record the slab walk reads -- copies of its medium's values and
 * its own two bounds: (mu_t, 1/mu_t, z_lo, z_hi, absorb, dep, 2g, 1-g, 1-g^2, 1+g^2, 1/(2g), n). */
int lt_layer_records(const lt_medium* media, int n_media, int quantity, const double* z_bounds, const int32_t* medium_idx,
                     int n_layers, int f32, void* media_out, void* zb_out, void* rec_out);
/* voxel grid (tally) -- role of Scene.image (scene.py:66).  C-order
 * [nz][ny][nx]; allocates and zeroes the device grid and the counters. */
int lt_set_grid(lt_ctx* ctx, int nx, int ny, int nz, const double origin[3],
                const double voxel[3], int tally_dtype);
/* source -- role of sample_light (light_samples.py:90-116).  start_medium:
 * medium id the photon starts in (mesh scenes; ignored for layers). */
int lt_set_source(lt_ctx* ctx, int type, const double pos[3], const double dir[3],
                  const double* extra, int start_medium);
/* cap on a photon's steps: a photon alive after that many goes to w_capped with its weight (0: where it is emitted). */
int lt_set_max_steps(lt_ctx* ctx, uint32_t max_steps);
/* Experiment knobs -- tuning constants and diagnostic switches that tests and measurement tools vary; results do not
 * depend on any of them (the tests hold that down bit for bit, for the f64 and for the f32 walks: a shortcut in front of a
 * surface query may only decline what the query itself would decline, so each compares with margins that cover the rounding
 * of its own operands in walk precision -- the f32 plane pre-test with a slack that grows with |a - o| and with the
 * triangle's conditioning, LT_FN_PLANE_REACH).  value < 0 restores the built-in default.  Each knob is
 * seeded ONCE, in lt_create, from the environment variable LT_<KEY IN CAPITALS>; the library reads the environment
 * nowhere else.  Keys:
 *   query_min          meshes in LDS: lanes a wave gathers before it serves their surface queries; meshes beyond LDS:
 *                      answered-but-untested queries that trigger a drain of the candidate queue            (1..64)
 *   log_bits2, log_hot two-pass partition: width of the second digit; cap on the number of hot tiles (0: plain two-pass)
 *   overlap_walk_bpc   workgroups per CU of a walk that shares the device with another lane's reduction     (1..8)
 *   diag_no_tally      time the walk without deposition;   log_timing  print per-stage device times of every launch
 *   tail_split         slab walks in log mode: 0 = the whole walk in one kernel; default = split (a wave hands its last
 *                      photons to the tail kernel when at most 32 lanes are alive) where a drain is exposed and the batch
 *                      has >= 512 photons per launched wave; n >= 2 = split with threshold n (<= 48) whatever the size
 *   part_alone         0 / 1: pin the partition build that shares the CU with a walk / the one for an otherwise idle device
 *   serial_walks       1: WALK TRAIN -- the walk kernels of every context of this device that sets the knob run one after
 *                      another (each waits for the end of the one enqueued before it; the log reductions stay on their own
 *                      streams).  For hosts that keep several jobs in flight: launch each walk at three of the four resident
 *                      workgroups per CU (lt_set_launch_config(3, 256)) and the free quarter of the register file carries the
 *                      reduction of the job in front (bench.py's walk_train regime)
 *   render_lds_tables  0: lt_render_surface reads the scene tables from global memory even where they fit LDS (tests: the two
 *                      kernels give the same image bit for bit)
 *   -- taking effect when the mesh tables are next built (lt_set_mesh + launch / query):
 *   march_cells        march grid: cells along the longest axis
 *   clearance_cells    clearance grid of meshes in LDS: cells along the longest axis
 *   no_march, no_clearance, no_near_lists   switch the shortcut off (every query then takes the slower exact path)
 *   force_march        meshes that fit LDS take the march grid and walk_kernel_m all the same (measurement) */
int lt_set_tuning(lt_ctx* ctx, const char* key, int64_t value);
/* LT_QUANTITY_*; applies to subsequent launches (the grid is NOT rescaled: zero it when switching) */
int lt_set_tally_quantity(lt_ctx* ctx, int quantity);
/* launch geometry: resident workgroups per CU and threads per workgroup
 * (multiples of 64).  0 keeps the default. */
int lt_set_launch_config(lt_ctx* ctx, int blocks_per_cu, int threads_per_block);

/* how deposits reach the grid.  LT_MODE_ATOMIC: one no-return global atomic per
 * deposit record.  LT_MODE_LOG: the walk appends records to a coalesced log in
 * HBM which is radix-partitioned by grid tile and reduced tile by tile in LDS
 * (no global atomics); photons are traced in batches sized to log_bytes, the
 * budget for all deposit logs of the ctx and their ping-pong copies (0 restores
 * the default: a quarter of the device memory, at most 64 GiB).  A log that turns
 * out too small diverts the excess records to atomics -- speed, never
 * correctness (lt_last_log_info reports how many).  The first launch of a new
 * scene traces a 16384-photon pilot batch and reads its record rate back (a few
 * ms on the host) so that logs and batches are sized from a measurement.
 * Results are identical for the u64 fixed-point tally and equal up to summation
 * order for float tallies.  Table RNG, vertex capture and grids beyond 65536
 * tiles (2^30 voxels) use the atomic path. */
#define LT_MODE_ATOMIC 0
#define LT_MODE_LOG 1
#define LT_MODE_AUTO 2 /* default: LOG whenever the launch can use it (no RNG table, no vertex capture, grid within the tile index range, free HBM), ATOMIC otherwise */
int lt_set_tally_mode(lt_ctx* ctx, int mode, uint64_t log_bytes);
/* optional: allocate the deposit log(s) for launches of up to n_photons now (otherwise the first launch does it) */
int lt_reserve_log(lt_ctx* ctx, uint64_t n_photons);
/* Overlap inside ONE lt_launch (log mode).  lanes = 2: the launch is cut into
 * sub-batches that alternate between two streams of the ctx, each with its own
 * deposit log, so that the bandwidth-bound reduction of batch k runs beside the
 * VALU-bound walk of batch k+1 (role of Numba's thread pool working through one
 * render_scene call, path_tracing_fix1.py:139-148: the caller still makes one
 * call).  lanes = 1: one stream, batches back to back.  lanes = 0 (default):
 * launches of >= 2^21 photons whose geometry the caller has not pinned
 * (lt_set_launch_config) try both once and keep the faster.  The ctx stream
 * joins both lanes before lt_launch returns, so everything ordered on lt_stream
 * (readback, lt_reduce_grid, lt_zero_tally) stays ordered.  The u64 fixed-point
 * grid is bit-identical for every setting. */
int lt_set_overlap(lt_ctx* ctx, int lanes);

/* ---- run --------------------------------------------------------------- */
/* role of render_scene (path_tracing_fix1.py:139-169): trace photons
 * [photon_offset, photon_offset + n_photons) asynchronously on the ctx stream,
 * ACCUMULATING into the grid and counters.
 *   rng_table == NULL : rocRAND XORWOW, state re-seeded per photon from
 *                       (seed, photon id) -- results do not depend on launch
 *                       geometry or on which rank traces which id range.
 *   rng_table != NULL : "table RNG" of the reference (scene.py:68-69,
 *                       path_tracing_fix1.py:28-29): host array
 *                       [n_photons][table_steps][4] of uniforms in [0,1),
 *                       addressed by (photon - photon_offset, step). */
int lt_launch(lt_ctx* ctx, uint64_t n_photons, uint64_t photon_offset, uint64_t seed,
              const double* rng_table, uint64_t table_steps, uint32_t flags);
int lt_sync(lt_ctx* ctx);
/* milliseconds of device time spent in the transport kernel by the last
 * lt_launch (HIP events on the ctx stream); valid after lt_sync. */
int lt_last_kernel_ms(lt_ctx* ctx, double* ms);
int lt_zero_tally(lt_ctx* ctx); /* zero grid + counters (async)           */
/* device milliseconds per stage, summed over the batches (and lanes) of the last
 * log-mode lt_launch: [0] walk kernel, [1] scan, [2] partition pass(es), [3] tile
 * reduce (with two lanes the stages of different batches overlap in time);
 * deposit records and batches of that launch. */
int lt_last_log_stages(lt_ctx* ctx, double ms_out[4], uint64_t* records, uint64_t* batches);
/* bookkeeping of the last log-mode lt_launch (blocks until it has finished): records written to the
 * deposit log, records that found it full and went to the grid as atomics, batches, lanes used */
int lt_last_log_info(lt_ctx* ctx, uint64_t* records, uint64_t* overflow_records, uint64_t* batches, int* lanes);
/* grids of more than 1024 tiles (a tile = 32 x 32 x 16 voxels) take two partition passes; once a tile histogram of
 * the scene is known (the pilot batch), the tiles that hold most records ("hot") leave the first pass in their final
 * form and only the rest goes through the second.  Reports, for the last log-mode lt_launch (blocking): how many tiles
 * were hot (0: plain two-pass or one-pass form) and the record count of the pilot histogram that made a tile hot.
 * lt_set_tuning("log_hot", n) caps the number of hot tiles (0 switches the form off). */
int lt_last_log_hot_tiles(lt_ctx* ctx, uint32_t* hot_tiles, uint32_t* threshold);

/* ---- readback ---------------------------------------------------------- */
/* blocking D2H of the raw tally ([nz][ny][nx], dtype as set) */
int lt_read_grid(lt_ctx* ctx, void* host_out, size_t bytes);
/* blocking D2H, converted to float64 absorbed weight per voxel */
int lt_read_grid_f64(lt_ctx* ctx, double* host_out, size_t n_voxels);
/* the inverse of lt_read_grid: blocking H2D of a raw tally ([nz][ny][nx], dtype as set, bytes = the grid's size) on the ctx
 * stream.  Overwrites the grid and leaves the counters as they are: restores a saved tally so that further launches
 * accumulate onto it.  LT_E_STATE without a grid, LT_E_INVALID on a size mismatch. */
int lt_write_grid(lt_ctx* ctx, const void* host_in, size_t bytes);
int lt_read_counters(lt_ctx* ctx, lt_counters* out);

/* ---- sums of the tally, taken on the device ------------------------------ */
/* What most users want from a run is far smaller than the grid: absorbed weight against depth, a projection, the
 * cylindrical map A(r, z).  The two calls below read the grid once in HBM and return a few KiB; both run on the ctx stream
 * (ordered behind earlier launches, as lt_read_grid is) and block until the output is filled.  Device memory beyond the
 * grid: partial sums and the output, in the ctx's scratch buffers.
 *   out      (required) f64 weight per bin, in the units of lt_read_grid_f64
 *   raw_out  (may be NULL; non-NULL only with LT_TALLY_U64FX, else LT_E_INVALID) the exact integer sums
 * LT_TALLY_U64FX: summed in integers, out = (double)raw * 2^-40 -- independent of the order, bit-reproducible.  The integer
 * sums wrap modulo 2^64: ONE BIN holds at most 2^24 = 1.68e7 units of weight, the bound stated above for a voxel.
 * LT_TALLY_F32 / LT_TALLY_F64: every voxel is widened to f64 and summed in f64.
 * LT_E_STATE without a grid. */

/* Sum the grid over the axes that are NOT kept.  keep_mask bits: 1 = x, 2 = y, 4 = z.  out is C-order over the kept axes in
 * z, y, x order: 4 -> [nz] (the depth profile), 3 -> [ny][nx], 5 -> [nz][nx], 6 -> [nz][ny], 1 -> [nx], 2 -> [ny], 0 -> one
 * number, the grid total.  7 (that is lt_read_grid) or any other bit: LT_E_INVALID.
 * Float tallies too are summed in a FIXED ORDER (partial sums, then a finishing pass; the order depends on the grid's shape
 * alone): two calls on an unchanged grid return identical bits. */
int lt_tally_sum_axes(lt_ctx* ctx, int keep_mask, double* out, uint64_t* raw_out);
/* Per z, sum the (y, x) columns bin by bin.  bin_of_column: host array [ny][nx], a bin in 0 .. n_bins-1 per column or -1 to
 * leave the column out (any other value: LT_E_INVALID).  out [nz][n_bins]: for every z the sum of the voxels whose column
 * carries that bin; a bin with no column is 0.  1 <= n_bins <= 4096; more: LT_E_UNSUPPORTED.  With a table of
 * lt_radial_bins this is the r-z map; with a 0 / -1 mask, any region of interest.
 * Float tallies are added into per-workgroup bins with LDS atomics: the result may differ from call to call in the last bits
 * (by the usual bound for a sum of n non-negative terms, n 2^-53 relative); the u64 fixed-point result is exact. */
int lt_tally_sum_columns(lt_ctx* ctx, const int32_t* bin_of_column, int n_bins, double* out, uint64_t* raw_out);
/* The table of lt_tally_sum_columns for rings about an axis parallel to z.  Pure host code: no ctx, no device.  For the
 * column (iy, ix) of an nx x ny grid, each line ONE IEEE double operation per operator (a NumPy restatement gives the same
 * integers):
 *     xc = origin_x + (ix + 0.5) * voxel_x          dx = xc - centre_x          (likewise yc, dy)
 *     r = sqrt(dx * dx + dy * dy)                    bin = (int)floor(r / dr),   any bin >= nr becomes nr
 * bins_out [ny][nx] holds 0 .. nr: nr + 1 bins, the last collecting everything beyond nr * dr, so that the map's total is the
 * grid's.  dr <= 0, nr < 1 or non-positive dimensions: LT_E_INVALID. */
int lt_radial_bins(int nx, int ny, const double origin_xy[2], const double voxel_xy[2], const double centre_xy[2], double dr,
                   int nr, int32_t* bins_out);

/* ---- parts of the tally: boxes, slices and coarser voxels ------------------ */
/* A box of the grid, summed in blocks of bin[0] x bin[1] x bin[2] voxels: with bin = (1, 1, 1) a sub-volume or, one voxel
 * thick, a slice (the plane through the beam); over the whole grid with bin > 1, the same volume at a coarser voxel size.  What
 * lt_tally_sum_axes cannot give (it sums whole axes: the central plane is not a projection), without moving the grid to the host.
 *   lo, size, bin   x, y, z order: the box's first voxel, its extent in voxels, the grid voxels per output voxel along each axis
 *   out             C-order [oz][oy][ox] with o[a] = ceil(size[a] / bin[a])
 * Output voxel (k, j, i) is the sum of the grid voxels with lo_z + k bz <= z < min(lo_z + (k + 1) bz, lo_z + size_z), likewise
 * in y and x: the LAST BLOCK of an axis is clipped to the box, never padded (a bin beyond the box gives one block).
 * Units and raw_out as for the sums above: out is f64 weight; raw_out (may be NULL; non-NULL only with LT_TALLY_U64FX, else
 * LT_E_INVALID) the exact integer sums, out = (double)raw * 2^-40, wrapping modulo 2^64 -- ONE OUTPUT VOXEL holds at most 2^24
 * units of weight.  Float tallies are widened to f64 and summed in f64.  No atomics; the order of every sum follows from (grid
 * shape, lo, size, bin) alone: the same call on an unchanged grid returns identical bits, for float tallies too.  With bin = (1,
 * 1, 1) an output voxel is the grid voxel converted exactly (an f64 tally: bit for bit), and the whole grid so read equals
 * lt_read_grid_f64.
 * Runs on the ctx stream behind earlier launches (as lt_read_grid is ordered), blocks until out is filled, and leaves the grid,
 * the counters and the statistics untouched.  Device memory beyond the grid: the output (and the integer sums if asked for) in
 * the ctx's scratch buffers; no partial sums.  Blocks below 512 voxels with bin_x <= 16 are summed by lanes that follow x (16
 * bytes each, the rows of a block in registers, the bin_x neighbours through LDS); larger ones by one workgroup per output voxel.
 * LT_E_STATE without a grid.  LT_E_INVALID: a NULL lo, size, bin or out; any lo < 0, size < 1 or bin < 1; a box that leaves the
 * grid on any axis (lt_last_error names the axis and the value); raw_out with a float tally. */
int lt_tally_box(lt_ctx* ctx, const int32_t lo[3], const int32_t size[3], const int32_t bin[3], double* out, uint64_t* raw_out);

/* ---- the tally convolved in x and y: the response to a beam of finite width ------ */
/* The tally of a pencil beam on a laterally uniform medium (a layered slab) is the medium's response G(x, y, z); the response
 * to a beam of profile S(x, y) is the convolution of G with S in x and y, plane by plane -- one traced run serves any number
 * of beam sizes.  With W[z][y][x] the tally as weight (the units of lt_read_grid_f64: a u64 fixed-point element is
 * (double)raw * 2^-40, an f32 element is widened) and W = 0 outside the grid,
 *     out[z - z0][y][x] = sum over j, i of taps[j][i] * W[z][y - (j - kh/2)][x - (i - kw/2)]      for z0 <= z < z0 + nz_out
 * -- a true convolution: the part of the beam displaced by (i - kw/2, j - kh/2) columns adds the pencil response displaced by the
 * same amount.  LIMIT: weight that would have come from beyond the grid's edge is missing -- the grid has to hold G plus the
 * beam, or the result is too small near the edges (never too large: the taps are non-negative).
 * Every tap is finite and >= 0 (a beam profile has no other kind; the error bound of the sums rests on it), every tap count is
 * odd and >= 1.  All three calls run on the ctx stream behind earlier launches, block until out is filled, and leave the grid,
 * the counters and the statistics untouched.  Everything is computed in f64 with fused multiply-adds, without atomics, in an
 * order that follows from the shapes alone: the same call on an unchanged grid returns identical bits, and a plane's bits do
 * not depend on z0 / nz_out.  Device memory beyond the grid: the output planes asked for (and for the separable form one
 * intermediate of the same size) in the ctx's scratch buffers -- nz_out is the means of staying small: one plane of a 512^3
 * grid is 2 MiB.
 * LT_E_STATE without a grid.  LT_E_INVALID: a tap that is negative, NaN or infinite; an even tap count or one below 1; a NULL
 * pointer; z0 < 0, nz_out < 1 or z0 + nz_out > nz; a column outside the grid; n_columns < 1.  LT_E_UNSUPPORTED: a tap count or
 * column count above the limit (the message names the number). */

/* taps [kh][kw], kh and kw odd, 1 .. 63; out [nz_out][ny][nx].  One workgroup per 32 x 32 output tile holds the tile and its
 * halo in LDS; a tile whose input region holds nothing costs its read alone. */
int lt_tally_convolve(lt_ctx* ctx, const double* taps, int kh, int kw, int z0, int nz_out, double* out);
/* The same with taps[j][i] = taps_y[j] * taps_x[i], as two one-dimensional passes -- x first, into an intermediate, then y: kw + kh
 * multiply-adds per voxel instead of kw * kh (the intermediate is rounded: the result is that of the two passes, not bit for bit
 * that of the outer product).  kh and kw odd, 1 .. 255. */
int lt_tally_convolve_sep(lt_ctx* ctx, const double* taps_x, int kw, const double* taps_y, int kh, int z0, int nz_out, double* out);
/* The convolved value at listed columns only, for every z: columns [n_columns][2] = (ix, iy) inside the grid, 1 <= n_columns <=
 * 4096; out [nz][n_columns].  The depth profile on the beam's axis, or a lateral profile, in a few KiB and without a grid in
 * between: the convolution's counterpart of lt_tally_sum_columns.  Taps as for lt_tally_convolve. */
int lt_tally_convolve_at(lt_ctx* ctx, const double* taps, int kh, int kw, const int32_t* columns, int n_columns, double* out);

/* ---- statistical error of the tally, from batch moments on the device --- */
/* How far can a voxel's number be trusted?  Trace the photons in N batches of EQUAL size and close every batch with
 * lt_stats_fold.  With statistics on the ctx owns two more device buffers of the grid's extent: `prev`, the grid as it stood at
 * the last fold (the tally's own type), and `m2` (f64), the sum over the closed batches of the squared batch contribution.
 * A fold does, per voxel (m2 + d * d is one rounded multiply, then one rounded add -- no fused multiply-add):
 *     d = grid - prev     LT_TALLY_U64FX: the integer difference, then (double)diff * 2^-40;  f32 / f64: (double)grid - (double)prev
 *     m2 = m2 + d * d     prev = grid
 * The estimator is that of batch means.  With S1 = prev in the units of lt_read_grid_f64, each line a single IEEE double
 * operation (a NumPy restatement gives the same bits up to the rounding of its divide and square root):
 *     S1 == 0 -> NaN (no estimate)       q = (N * m2) / (S1 * S1)       v = q - 1, v < 0 -> 0       R = sqrt(v / (N - 1))
 * R is the relative standard error of the mean over the N batches: 1 where a single batch contributed, 0 where all of them
 * contributed equally.  It means what it says only if the batches are of equal size (the same number of photons each); results
 * do not depend on how a batch's photon ids were split into launches.  Voxels of one batch are correlated, so the error of a
 * SUM of voxels (a depth profile) does not follow from the per-voxel moments: take lt_tally_sum_axes after every fold and keep
 * the moments of the per-batch sums on the host.
 * While statistics are on: lt_zero_tally also zeroes prev, m2 and N; lt_set_grid turns statistics off; lt_write_grid stays
 * legal (the next fold books the difference as a batch); lt_reduce_grid across ranks is NOT supported (prev and m2 stay
 * local: the moments would no longer belong to the grid).  With statistics off no other call changes in any way.
 * Every call below: LT_E_STATE while statistics are off, LT_E_INVALID on a NULL output or a wrong n_voxels. */

/* on != 0: allocate and zero prev and m2, N = 0 (again, if statistics were on already).  LT_E_STATE without a grid, or if
 * anything was launched into or written to the grid since the last lt_set_grid / lt_zero_tally (prev is the grid only while
 * both are zero); LT_E_NOMEM if the device cannot hold 8 + sizeof(tally element) more bytes per voxel.
 * on == 0: release the buffers (never an error). */
int lt_stats_enable(lt_ctx* ctx, int on);
/* Close a batch: N += 1.  Asynchronous, on the ctx stream, ordered behind earlier launches exactly as lt_read_grid is.  A pure
 * streaming pass: a 16-byte group whose grid and prev bits are equal writes nothing and does not read m2, so a fold of a traced
 * grid costs about two reads of the grid.  A fold with nothing traced since the last one is a batch of zeros.  A grid that
 * holds LESS than prev (a smaller tally was written over it) is the caller's error: the result is unspecified. */
int lt_stats_fold(lt_ctx* ctx);
/* N, the number of closed batches */
int lt_stats_batches(lt_ctx* ctx, uint64_t* n_out);
/* blocking D2H of m2, [nz][ny][nx] f64 */
int lt_stats_read_m2(lt_ctx* ctx, double* out, size_t n_voxels);
/* blocking: R per voxel, [nz][ny][nx] f64 (NaN where S1 == 0), through the ctx's scratch buffer as lt_read_grid_f64 goes.
 * LT_E_STATE if N < 2. */
int lt_stats_read_relerr(lt_ctx* ctx, double* out, size_t n_voxels);
/* blocking: "how many voxels, holding how much of the weight, are below x % error" without reading a grid back.  edges:
 * 1 <= n_edges <= 63 finite, non-negative, strictly ascending values (anything else LT_E_INVALID; more than 63
 * LT_E_UNSUPPORTED).  The class of a voxel is the number of edges <= R -- the R lt_stats_read_relerr returns for it, computed
 * by the same device function.  voxels_out, weight_out (both required) and raw_weight_out [n_edges + 2]: per class 0 .. n_edges
 * the voxels and the sum of their S1; the last entry is the class of the voxels with S1 == 0, whose weight is 0.  The voxel
 * counts, and with LT_TALLY_U64FX the weights, are integer sums: exact.  Float tallies are widened to f64 and added into
 * per-workgroup bins with LDS atomics, then in a fixed order: the last bits may differ from call to call.  raw_weight_out: may
 * be NULL; non-NULL only with LT_TALLY_U64FX (else LT_E_INVALID), the integer sums.  LT_E_STATE if N < 2. */
int lt_stats_summary(lt_ctx* ctx, const double* edges, int n_edges, uint64_t* voxels_out, double* weight_out,
                     uint64_t* raw_weight_out);

/* ---- results by region: label volume, per-label totals, dose-volume histograms ------ */
/* "How much did THIS structure absorb, where is its hottest voxel, what share of its volume got at least dose D?" -- without
 * reading the grid back.  A label volume gives every voxel a region: labels [nz][ny][nx], one byte per voxel, each 0 ..
 * n_labels - 1 or LT_LABEL_NONE for a voxel that is left out of everything; 1 <= n_labels <= 64.  lt_set_labels copies the volume
 * into a device buffer the ctx owns (1 byte per voxel) and blocks until it has left the caller's array; labels == NULL releases
 * it.  lt_set_grid drops the labels; lt_zero_tally, lt_write_grid and launches leave them alone.  WITHOUT labels both result
 * calls treat the whole grid as label 0 with n_labels = 1: a plain histogram of the tally and a peak finder, with no setup.
 * LT_E_STATE without a grid.  LT_E_INVALID: n_voxels that is not the grid's, n_labels outside 1 .. 64, a byte that is neither
 * below n_labels nor LT_LABEL_NONE (checked on the host; lt_last_error names the first such flat index and its value). */
#define LT_LABEL_NONE 255
int lt_set_labels(lt_ctx* ctx, const uint8_t* labels, size_t n_voxels, int n_labels);
/* n_labels_out: the n_labels in force, 0 when no labels are set */
int lt_labels_info(lt_ctx* ctx, int* n_labels_out);
/* Per label, [n_labels] each: weight_out the sum of its voxels in the units of lt_read_grid_f64; raw_out (may be NULL; non-NULL
 * only with LT_TALLY_U64FX, else LT_E_INVALID) the exact integer sum, wrapping modulo 2^64, weight_out = (double)raw * 2^-40;
 * voxels_out its voxels; filled_out those that are not zero; peak_out its largest voxel, converted exactly as lt_read_grid_f64
 * converts a voxel; peak_index_out the LOWEST flat index (z * ny + y) * nx + x among its voxels that hold the peak -- an all-zero
 * label reports its first voxel, a label without voxels index -1 and peak 0.  All but raw_out are required.  Counts, peaks,
 * indices and the integer sums are exact; float weights as for lt_tally_histogram.  One pass over the grid and the labels; the
 * workgroups that saw a label's peak read their part once more for its index (a tally is taken to be >= 0). */
int lt_tally_label_sums(lt_ctx* ctx, double* weight_out, uint64_t* raw_out, uint64_t* voxels_out, uint64_t* filled_out,
                        double* peak_out, int64_t* peak_index_out);
/* The histogram of the tally per label.  edges as for lt_stats_summary: 1 <= n_edges <= 63 finite, non-negative, strictly
 * ascending values (anything else LT_E_INVALID; more than 63 LT_E_UNSUPPORTED).  With v the voxel as weight (LT_TALLY_U64FX:
 * (double)raw * 2^-40, one rounding; f32 widened) its class is the number of edges <= v.  voxels_out, weight_out (both required)
 * and raw_weight_out [n_labels][n_edges + 1]: the voxels per (label, class) and the sum of their values.  The voxel counts, and
 * with LT_TALLY_U64FX the weights, are integer sums: exact.  Float tallies are widened to f64 and added into per-workgroup bins
 * with LDS atomics, then in a fixed order: the last bits may differ from call to call.  raw_weight_out: may be NULL; non-NULL only
 * with LT_TALLY_U64FX (else LT_E_INVALID).  The cumulative dose-volume histogram V(>= edge k) is the reverse cumulative sum of a
 * label's row on the host.
 * Both result calls run on the ctx stream behind earlier launches (as lt_read_grid is ordered), block until the outputs are
 * filled, leave the grid, the counters, the statistics and the labels untouched, and keep their partial sums in the ctx's
 * scratch buffers.  LT_E_STATE without a grid, LT_E_INVALID on a NULL required pointer. */
int lt_tally_histogram(lt_ctx* ctx, const double* edges, int n_edges, uint64_t* voxels_out, double* weight_out,
                       uint64_t* raw_weight_out);

/* ---- the tally along rays: line integrals, maxima, the first voxel above a threshold ------ */
/* Everything above is locked to the grid's axes.  These two calls read the tally along ARBITRARY rays -- an oblique projection,
 * the integral along a tilted fibre, a maximum-intensity projection, "how deep does the 10 % isodose reach, seen from here" --
 * and return a few numbers per ray; the grid stays on the device.  One lane per ray steps voxel to voxel through the grid.
 *   W[v]         the voxel as weight, converted exactly as lt_read_grid_f64 converts it.
 *   voxel boxes  voxel (i, j, k) is the half-open box [origin_a + i voxel_a, origin_a + (i + 1) voxel_a) on every axis: the walk's
 *                floor rule.
 *   rays         o + t d for t_lo <= t <= t_hi; d of any non-zero finite length; lengths are geometric, (t2 - t1) |d|.
 *   integral     sum over the voxels v of W[v] l_v, with l_v the length of the ray's segment inside v: weight x length.
 *   max          the largest W among the voxels with l_v > 0 (LT_TALLY_U64FX: the integers are compared, the largest converted
 *                once); max_index the flat index (z ny + y) nx + x of the FIRST such voxel along the ray that holds it.  A ray that
 *                crosses no voxel: max 0, index -1.
 *   first        first_index: the first voxel along the ray with l_v > 0 and W >= threshold (the comparison is on the converted
 *                double, as lt_tally_histogram classes a voxel); first_t: the parameter at which the ray enters it, never below
 *                t_lo, in the units of the d given.  No such voxel: +inf and -1, as lt_intersect_rays reports a miss.  threshold =
 *                0 therefore returns the entry into the grid.
 *   d_a == 0     the index on that axis is floor((o_a - origin_a) / voxel_a) throughout; outside 0 .. n_a - 1 the ray misses.
 *   grazing      whether a voxel that the ray only grazes -- a corner, an edge, a chord within rounding of zero -- is visited is
 *                unspecified; what it adds to the integral is negligible either way.
 * Arithmetic: f64 throughout, every operation rounded on its own (no fused multiply-add).  The parameter of a grid plane is the
 * quotient ((origin_a + p voxel_a) - o_a) / d_a of the plane's own coordinate, never a repeated addition: the error does not grow
 * with the grid.  No atomics; a ray is summed in the order it is walked: the same call on an unchanged grid returns identical
 * bits, for all three tally types.
 * Any output pointer may be NULL (at least one is not); only what is asked for is computed.  Both calls run on the ctx stream
 * behind earlier launches (as lt_read_grid is ordered), block until the outputs are filled, and leave the grid, the counters, the
 * statistics and the labels untouched.  Rays and outputs live in the ctx's scratch buffers.
 * LT_E_STATE without a grid.  LT_E_INVALID, all checked on the host (lt_last_error names the first offending ray): no output asked
 * for; a NULL origins, dirs, camera, xs or ys; n, width or height < 1; a non-finite origin or direction, or d = 0; t_lo < 0 or not
 * finite, or t_hi <= t_lo (t_hi = +inf is legal); a first-crossing output with a threshold that is negative or not finite. */

/* origins, dirs [n][3]; t_range [n][2] = (t_lo, t_hi) per ray, or NULL = [0, +inf); every output [n] */
int lt_tally_rays(lt_ctx* ctx, const double* origins, const double* dirs, const double* t_range, size_t n, double threshold,
                  double* integral_out, double* max_out, int64_t* max_index_out, double* first_t_out, int64_t* first_index_out);
/* The rays of the pinhole camera of lt_render_surface, without its jitter: pixel (i, j) has o = camera and d = (xs[j] - o.x,
 * ys[i] - o.y, f_distance - o.z), t in [0, +inf); every output [height][width].  The same __device__ traversal as lt_tally_rays:
 * the result equals lt_tally_rays on those rays built on the host, bit for bit.  A wave takes an 8 x 8 pixel tile. */
int lt_tally_view(lt_ctx* ctx, int width, int height, const double camera[3], double f_distance, const double* xs, const double* ys,
                  double threshold, double* integral_out, double* max_out, int64_t* max_index_out, double* first_t_out,
                  int64_t* first_index_out);

int lt_grid_device_ptr(lt_ctx* ctx, void** ptr, size_t* bytes);
int lt_counters_device_ptr(lt_ctx* ctx, void** ptr, size_t* bytes);
void* lt_stream(lt_ctx* ctx); /* hipStream_t of the ctx */
/* sum-reduce grid + counters over an RCCL communicator (ncclComm_t), on the
 * ctx stream; root < 0 = all-reduce.  librccl is loaded on first use. */
int lt_reduce_grid(lt_ctx* ctx, void* nccl_comm, int root);

/* ---- geometry / sampling queries on the device ------------------------- */
/* These run the SAME __device__ functions the walk uses, one lane per query,
 * so the reference's per-function behaviour can be checked in isolation. */

/* nearest hit of n rays against the ctx mesh -- role of hit_object /
 * intersect_bvh (utils.py:53-68, bvh_new.py:414-482), predicate
 * EPSILON < t < tmax.  prim_out = -1, t_out = +inf when nothing is hit.
 * use_bvh = 0: brute force over all triangles; 1: the flattened BVH; 2: the march grid as the walk uses it for meshes beyond
 * LDS (wave-cooperative: lanes march their rays through the grid, the whole wave tests the candidates; built on request for
 * smaller meshes); 3: the same march lane by lane; 4: the BVH front to back -- the child on the ray's side of the split plane
 * first, the reference's order (bvh_new.py:455-458), threaded per direction sign pattern so that it needs no stack: what the
 * surface renderers use (a BVH of more than 32767 nodes has no front-to-back tables: 4 then searches it in storage order,
 * as 1 does).  All five give the same answer bit for bit. */
int lt_intersect_rays(lt_ctx* ctx, const double* origins, const double* dirs,
                      const double* tmax, size_t n, int use_bvh, int32_t* prim_out,
                      double* t_out);
/* pairwise Moller-Trumbore -- role of triangle_intersect
 * (intersects.py:46-104).  tris [n][3][3]; t_out = NaN for "None". */
int lt_triangle_intersect(lt_ctx* ctx, const double* origins, const double* dirs,
                          const double* tris, size_t n, double* t_out);
/* pairwise slab test -- role of intersect_bounds (intersects.py:179-196).
 * boxes [n][2][3] (min,max); hit_out 0/1. */
int lt_intersect_bounds(lt_ctx* ctx, const double* origins, const double* dirs,
                        const double* tmax, const double* boxes, size_t n,
                        int32_t* hit_out);
/* sampling helpers, n independent evaluations each:
 *  LT_FN_HG_PDF       in: cos_theta, g            out: [1] henyey_greenstein (medium_samples.py:14-16)
 *  LT_FN_HG_SAMPLE    in: xi, g                   out: [1] deflection cosine (Appendix C.6)
 *  LT_FN_ONB          in: n[3]                    out: [6] v2,v3 (utils.py:72-80)
 *  LT_FN_DISK         in: u[2]                    out: [2] (utils.py:115-128)
 *  LT_FN_COSINE_HEMI  in: n[3], wi[3], u[2]       out: [4] dir, pdf (utils.py:132-161)
 *  LT_FN_REFLECT      in: v[3], n[3]              out: [3] (brdf.py:8-9)
 *  LT_FN_BOUNDARY     in: d[3], n[3], n1, n2      out: [5] R_fresnel, cos_t, refracted[3] (Appendix C.5)
 *  LT_FN_SPIN         in: u[3], cos_t, phi_xi     out: [3] rotated direction (Appendix C.6)
 * in/out are row-major [n][k]. */
#define LT_FN_HG_PDF 0
#define LT_FN_HG_SAMPLE 1
#define LT_FN_ONB 2
#define LT_FN_DISK 3
#define LT_FN_COSINE_HEMI 4
#define LT_FN_REFLECT 5
#define LT_FN_BOUNDARY 6
#define LT_FN_SPIN 7
#define LT_FN_WALK_MATH 8 /* in: x in (0,1]  out: [5] -ln x, sin 2 pi x, cos 2 pi x, sqrt x, 1/(1+x) -- the walk's f64 primitives */
#define LT_FN_WALK_MATH_RAW 9 /* in: k = a raw 32-bit draw (as a double)  out: [3] -ln u, sin 2 pi u, cos 2 pi u of u = (k + 1) 2^-32, by the forms the f64 XORWOW walk uses on the raw draw */
#define LT_FN_PLANE_REACH 10 /* in: o[3], d[3], tri[3][3], s, f32 (0 / 1)  out: [2] reach, t -- the mesh walk's plane pre-test (1: a hop of length s from o along d may reach the triangle's plane; 0: rejected without a triangle test) and the triangle test's own t (NaN: none), both in walk precision (f32 != 0: float) on the triangle record a launch uploads.  o, d, s are narrowed to float as given: pass values a float holds.  The pre-test is sound when no row has reach = 0 with 1e-6 < t < s */
#define LT_FN_HG_WALK 11 /* in: xi, f32 (0 / 1), then the 12 values of one medium record exactly as lt_layer_records returned them for that precision  out: [2] the deflection cosine as the walk takes it (clamped to [-1, 1]), in walk precision (f32 != 0: float; pass an xi a float holds), from the medium table (mesh walks) and from the layer record (slab walks) */
int lt_eval(lt_ctx* ctx, int fn, const double* in, size_t n, double* out);
/* first `count` raw 32-bit XORWOW outputs of photon `photon_id` under `seed`
 * (checks the per-photon seeding against the oracle's restatement) */
int lt_rng_raw(lt_ctx* ctx, uint64_t seed, uint64_t photon_id, uint32_t count,
               uint32_t* out);

/* ---- surface path tracing on the same mesh ------------ */
/* per-triangle surface record: the Material fields trace_path reads
 * (material.py:28-37; path_tracing_fix1.py:45-119) + PreComputedTriangle.is_light */
typedef struct lt_surface_material {
    double diffuse[3];   /* material.color.diffuse */
    double emission;
    double ior;
    double transmission;
    int32_t is_diffuse, is_mirror, is_light, pad_;
} lt_surface_material;

/* one point sample of the area light: role of Light (scene.py:12-17).
 * radiance = material.emission * material.color.diffuse (light_samples.py:56) */
typedef struct lt_point_light {
    double source[3];
    double normal[3];
    double radiance[3];
    double total_area;
} lt_point_light;

/* one entry per triangle of the current mesh (lt_set_mesh order) */
int lt_set_surface_materials(lt_ctx* ctx, const lt_surface_material* mats, int n_tris);
int lt_set_lights(lt_ctx* ctx, const lt_point_light* lights, int n);
/* role of render_scene + trace_path (path_tracing_fix1.py:18-169).  One lane
 * per pixel.  xs[width] / ys[height]: screen coordinates (np.linspace of
 * left..right / top..bottom, :141-142).  rand_0 / rand_1: the Scene tables
 * [H][W][S][D] (scene.py:68-69); rand_0 is updated in place with the +inf
 * markers the reference writes for unused bounces (:38,66,130).  light_choice
 * [H][W][S][D]: index of the light sample used by the shadow ray of that bounce
 * (the reference draws it with np.random.choice, light_samples.py:38).
 * image [H][W][3] is ACCUMULATED into: += 0.25 * clip(mean colour) (:166).
 * Any mesh size: the BVH is searched front to back (lt_intersect_rays form 4), in
 * storage order where it has more than 32767 nodes. */
int lt_render_surface(lt_ctx* ctx, int width, int height, int samples, int max_depth,
                      const double camera[3], double f_distance, const double* xs,
                      const double* ys, double* rand_0, const double* rand_1,
                      const int32_t* light_choice, double* image);
/* role of render_scene + trace_path of path_tracing_old.py:17-171, the recursive
 * integrator examples/LTS.ipynb calls: a diffuse hit recurses on the shared ray
 * and carries on from where the callee left it (:68-80), emission counts at
 * bounce 0 only (:45), roulette starts after bounce 3 (:127).  Same tables as
 * lt_render_surface, except that one path casts up to 2^max_depth - 1 shadow
 * rays: light_choice is [H][W][S][choices_per_sample] and the k-th shadow ray of
 * a sample (depth-first order) uses entry k mod choices_per_sample.
 * max_depth <= 24.  image [H][W][3] is OVERWRITTEN with clip(mean colour) (:167). */
int lt_render_surface_old(lt_ctx* ctx, int width, int height, int samples, int max_depth,
                          const double camera[3], double f_distance, const double* xs,
                          const double* ys, double* rand_0, const double* rand_1,
                          const int32_t* light_choice, int choices_per_sample, double* image);

/* ---- light sub-path vertices ("photon map" output) ----- */
/* Role of the Vertex record and of generate_light_subpaths / random_walk
 * (vertex.py:24-37, bdpt.py:18-147,258-268; both unrunnable in the reference):
 * besides depositing into the grid, the walk stores the first
 * max_vertices_per_photon vertices of every photon's path. */
#define LT_VERTEX_LIGHT 5        /* emission point (constants.py:22, Medium.LIGHT)     */
#define LT_VERTEX_REFLECTIVE 3   /* boundary event, reflected (Medium.REFLECTIVE)      */
#define LT_VERTEX_TRANSMISSIVE 4 /* boundary event, refracted / escaped                */
#define LT_VERTEX_VOLUME 7       /* interaction site in a medium (no reference value)  */
typedef struct lt_vertex {
    double point[3];     /* Vertex.point                                              */
    double direction[3]; /* direction of travel on arrival                            */
    double g_norm[3];    /* Vertex.g_norm: the light's normal (light_samples.py:104) / the interface normal facing
                            the arriving photon; zero inside a medium (bdpt.py:275: "on a surface if non-zero") */
    double throughput;   /* photon weight on arrival (Vertex.throughput, scalar)      */
    double pdf_pos;      /* emission vertex: 1 / light area (light_samples.py:100); pencil beam: 1; else 0 */
    double pdf_dir;      /* density of the direction the path LEAVES this vertex in: emission -- |cos| / pi
                            (light_samples.py:83), pencil beam: 1; medium -- the Henyey-Greenstein value
                            (medium_samples.py:14-16) of the sampled deflection; interface (a delta event) -- the
                            probability of the branch taken, R or 1 - R; 0 when the path ends here.  A path's
                            pdf_fwd[k] = pdf_dir[k-1] and pdf_rev[k] = pdf_dir[k+1] (bdpt.py:25-27,137; both
                            distributions are symmetric), in solid-angle measure                           */
    int32_t kind;        /* LT_VERTEX_* (Vertex.medium)                               */
    int32_t medium;      /* layer index (slabs) / medium id (meshes) on arrival       */
    uint32_t step;       /* photon-step index of the event (0 = emission)             */
    uint32_t pad_;
} lt_vertex;
/* 0 disables capture (default).  Applies to subsequent lt_launch calls. */
int lt_set_vertex_capture(lt_ctx* ctx, uint32_t max_vertices_per_photon);
/* vertices [n_photons][max_vertices_per_photon] and counts [n_photons] of the
 * LAST lt_launch (photon index = id - photon_offset); blocking D2H. */
int lt_read_vertices(lt_ctx* ctx, lt_vertex* vertices_out, uint32_t* counts_out, uint64_t n_photons);

/* What accelerates surface queries on the current mesh (built at the first launch / query after lt_set_mesh; this call
 * builds it if need be).  kind: 0 none (BVH only), 1 clearance grid with near-triangle lists (meshes whose tables fit
 * LDS), 2 march grid (meshes beyond LDS), 3 both (the f32 tables fit LDS, the f64 ones do not).  march_dims /
 * clearance_dims: cells along x, y, z (zeros if absent); march_entries: (cell, triangle) pairs in the candidate lists. */
int lt_mesh_accel_info(lt_ctx* ctx, int* kind, int march_dims[3], uint64_t* march_entries, int clearance_dims[3]);

/* device description for bench reports */
int lt_device_info(lt_ctx* ctx, char* name, size_t name_len, int* n_cus,
                   int* clock_mhz, size_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* LT_H_ */
