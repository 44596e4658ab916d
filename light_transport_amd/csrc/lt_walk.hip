// lt_walk.hip -- gfx950 (CDNA4) kernels of the photon-transport hot path: the walk kernels, their LDS layout, deposit code
// and variant dispatch, on the __device__ functions of lt_device.hpp.
//
// Design:
//   * one wavefront lane per live photon; photon state lives in VGPRs;
//   * persistent threads: the grid is sized to the resident capacity of the
//     chip and every wave loops, pulling PACKETS of photon ids from one global
//     counter (1 returning atomic per 64 photons) -- divergent path lengths are
//     absorbed by refilling dead lanes, not by launching more threads;
//   * dead lanes are found with a wave ballot and refilled by ballot rank
//     (v_mbcnt), four at a time (a refill costs the whole wave ~140 instructions);
//   * rocRAND XORWOW state per lane, re-seeded per photon from (seed, id) and
//     warmed up by 8 discarded outputs, so a photon's uniforms do not depend
//     on which lane / wave / GPU traces it;
//   * the kernel body lives in lt_walk_kernel.inc and is instantiated three
//     times: walk_kernel (slabs), walk_kernel_q (meshes: BVH queries batched per
//     wave, the one divergent block expensive enough to be worth waiting for)
//     and walk_kernel_m (meshes beyond LDS: queries marched through a grid);
//   * media, layer and BVH/triangle tables are staged once per workgroup into
//     LDS (all lanes read the same few entries: LDS broadcast);
//   * deposits: consecutive same-voxel deposits of a lane are merged in
//     registers; the surviving records go either to the grid with no-return
//     global atomics (f32 / f64 / u64 fixed point) or -- default for slabs --
//     into a coalesced deposit log that lt_logtally.hip partitions by grid tile
//     and reduces in LDS (the memory-side atomic unit, ~16e9 requests/s, was
//     the limiter; HBM streaming bandwidth is not); rare per-photon events go
//     to LDS counters;
//   * f64 arithmetic (the reference's dtype) with lean -ln / sincos / sqrt /
//     quotient primitives for the hot loop's restricted argument ranges.
// No MFMA: there is no dense contraction anywhere on this path.
//
// Reference citations: S/ = LightTransportSimulator/light_transport/src/.
#include "lt_device.hpp"
#include "lt_tally.hpp"

namespace ltk {

// ---------------------------------------------------------------------------
// tally: a deposit is accumulated in the tally's element type (TallyT, lt_tally.hpp) before it is sent to memory
// ---------------------------------------------------------------------------
template <int TALLY, typename R> LT_DEV typename TallyT<TALLY>::type tally_quantum(R dw)
{
    if constexpr (TALLY == LT_TALLY_U64FX) return (unsigned long long)((double)dw * LT_FX_SCALE + 0.5);
    else return (typename TallyT<TALLY>::type)dw;
}

template <int TALLY> LT_DEV void tally_add(void* grid, unsigned idx, typename TallyT<TALLY>::type v)
{
    if constexpr (TALLY == LT_TALLY_NONE) { asm volatile("" ::"v"(idx), "v"(v)); }
    else
        __hip_atomic_fetch_add(reinterpret_cast<typename TallyT<TALLY>::type*>(grid) + idx, v, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// LDS image of the scene tables
// ---------------------------------------------------------------------------
template <typename R> struct LdsLayout {
    size_t off_cnt, off_frame, off_media, off_zb, off_if, off_lm, off_lay, off_tris, off_nodes, off_links, off_hist, off_march, off_math, total;
    // Slab walks keep origin / inverse voxel size in registers (LT_INV_MODE 1), so the frame block's last nine values (bytes
    // 6 R ... 15 R of it) are theirs to use -- at offsets that are constants of the build, so a read is `ds_read ... offset:`
    // from the zero base the kernel holds for its LDS counters, and no layout moves:
    //   kSlabDim   the grid's three dimensions as u32 (16-byte aligned; f32: the frame block's last 12 bytes + 4 of its padding)
    //   kSlabCap   u64: photons that met the step cap (they are counted as stepping where the wave counts its live lanes)
    static constexpr size_t kCntBytes = 8 * sizeof(double), kFrame = (kCntBytes + 15) & ~(size_t)15;      // the counters lead, the frame block follows
    static constexpr size_t kSlabDim = kFrame + 48, kSlabCap = kFrame + (sizeof(R) == 8 ? 64 : 32);
    __host__ __device__ LdsLayout(int n_media, int n_layers, int n_tris, int n_nodes, unsigned n_hist = 0, size_t march_bytes = 0)
    {
        auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
        size_t o = 0;
        off_cnt = o;   o = al(o + kCntBytes);      // = kFrame
        off_frame = o; o = al(o + 15 * sizeof(R));     // frame of the source normal (area sources) + the grid's origin / inverse voxel / dimensions
        off_media = o; o = al(o + (size_t)n_media * sizeof(MedD<R>));
        off_zb = o;    o = al(o + (size_t)(n_layers + 1) * sizeof(R));
        off_if = o;    o = al(o + (size_t)(n_layers > 0 ? n_layers + 1 : 0) * sizeof(IfD<R>));
        off_lm = o;    o = al(o + (size_t)(n_layers > 0 ? n_layers : 1) * sizeof(int32_t));
        off_lay = o;   o = al(o + (size_t)(n_layers > 0 ? n_layers : 0) * sizeof(LayD<R>));      // slab walks: the per-layer step records
        off_tris = o;  o = al(o + (size_t)n_tris * sizeof(TriD<R>));
        off_nodes = o; o = al(o + (size_t)n_nodes * sizeof(NodeD<R>));
        off_links = o; o = al(o + (size_t)n_nodes * 16 * sizeof(int16_t));      // front-to-back link tables (8 patterns x first | after)
        off_hist = o;  o = al(o + (size_t)n_hist * sizeof(uint32_t));
        off_march = o; o = al(o + march_bytes);
        off_math = o;  o = al(o + (sizeof(R) == 8 ? kWalkMathTabBytes : 0));      // f64 walks: kWalkMathTab
        total = o;
    }
};

LT_DEV unsigned long long readlane64(unsigned long long v, int lane)
{
    unsigned lo = __builtin_amdgcn_readlane((unsigned)v, lane);
    unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// a * b + c for a, b < 2^24 (b wave-uniform) as v_mad_u32_u24.  The instruction is named because the compiler cannot be told:
// it does not know the factors' ranges, and where only the low bits of the result are kept it drops a mask on them (and HIP's
// __umul24 with it) and multiplies in 32 bits -- v_mad_u64_u32, with a 64-bit addend and result.  Both issue at 1.7 x the
// price of an integer add (tools/probes/int_mul_rate_probe.hip): the 24-bit form saves the register pairs, not issue time.
LT_DEV unsigned mad_u24(unsigned a, unsigned b, unsigned c)
{
    unsigned r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
    return r;
}

template <typename T> LT_DEV T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// light sub-path capture (f4): store vertex k of photon `rel` while k < max_vertices
template <typename R>
LT_DEV void record_vertex(const WalkParams& P, unsigned long long rel, unsigned& nv, R px, R py, R pz, R ux, R uy,
                          R uz, R w, int kind, int medium, unsigned step, R gx, R gy, R gz, R pdf_pos, R pdf_dir)
{
    if (nv < P.max_vertices) {
        lt_vertex* v = P.vertices + rel * (unsigned long long)P.max_vertices + nv;
        v->point[0] = (double)px; v->point[1] = (double)py; v->point[2] = (double)pz;
        v->direction[0] = (double)ux; v->direction[1] = (double)uy; v->direction[2] = (double)uz;
        v->g_norm[0] = (double)gx; v->g_norm[1] = (double)gy; v->g_norm[2] = (double)gz;
        v->throughput = (double)w; v->pdf_pos = (double)pdf_pos; v->pdf_dir = (double)pdf_dir;
        v->kind = kind; v->medium = medium; v->step = step; v->pad_ = 0;
        nv++;
        P.vertex_counts[rel] = nv;
    }
}

// One deposit record per lane (or none) leaves the lane's run-length accumulator.  Atomic route: a no-return
// global atomic.  Log route: the wave's records are compacted by ballot rank and appended, coalesced, to the wave's
// current log chunk (SoA: voxel index, value); a chunk is claimed with one returning atomic per kLogChunk records.
// If the log is exhausted the wave falls back to atomics, so a too-small log costs speed, never correctness.
// A lane without a record passes idx == kNoVoxel (its val is then not read).
// ROUTE: the slab walks are built per route (kRouteAtomic / kRouteLog: walk_kernel's ROUTE, chosen by launch_walk from
// P.log_idx), so a step holds one route's code and no test of which; the mesh walks test P.log_idx in every emit
// (kRouteRuntime: they sit at their register limits and keep the code they had).
constexpr int kRouteRuntime = 2;                  // beside Variant's kRouteAtomic / kRouteLog
constexpr unsigned kLogExhausted = 0xfffffffeu;   // lg_chunk: this wave has found the log full (0xffffffff: no chunk claimed yet)
constexpr unsigned kNoVoxel = 0xffffffffu;        // idx: no record

// the wave's chunk is full (or it has none yet): close it and claim the next of the group's chunks, or find the log exhausted
LT_DEV void log_claim(const WalkParams& P, unsigned& lg_cur, unsigned& lg_end, unsigned& lg_chunk)
{
    const int lane = threadIdx.x & 63;
    const unsigned grp = blockIdx.x & (kLogGroups - 1);
    if (lg_chunk < kLogExhausted && lane == 0) P.log_fill[lg_chunk] = lg_cur - lg_chunk * kLogChunk;
    unsigned c = 0;
    if (lane == 0) c = __hip_atomic_fetch_add(P.log_next + grp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c = grp + kLogGroups * __builtin_amdgcn_readfirstlane(c);     // the group's own chunks: see kLogGroups
    if (c < P.log_cap_chunks) { lg_chunk = c; lg_cur = c * kLogChunk; lg_end = lg_cur + kLogChunk; }
    else { lg_chunk = kLogExhausted; lg_cur = lg_end = 0; }
}

// log exhausted: back to the linear voxel index and a global atomic
template <int TALLY>
LT_DEV void log_spill(const WalkParams& P, unsigned idx, typename TallyT<TALLY>::type val, bool has, unsigned cnt)
{
    if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(P.log_overflow, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (has) {
        // (the divisors pass through an empty asm so that the reciprocal set-up of these divisions stays in this rare
        // branch: left visible as loop invariants it was hoisted in front of the walk's loop and parked in registers)
        unsigned ntx = P.log_ntx, nty = P.log_nty;
        asm volatile("" : "+s"(ntx), "+s"(nty));
        const unsigned tile = idx >> kTileShift, tx = tile % ntx, ty = (tile / ntx) % nty,
                       tz = tile / (ntx * nty);
        const unsigned vx = (tx << kTileBX) | (idx & 31u), vy = (ty << kTileBY) | ((idx >> 5) & 31u),
                       vz = (tz << kTileBZ) | ((idx >> 10) & 15u);
        tally_add<TALLY>(P.grid, (vz * (unsigned)P.ny + vy) * (unsigned)P.nx + vx, val);
    }
}

// the wave's records (mask m, cnt of them), compacted by rank, to records [lg_cur, lg_cur + cnt) of its chunk
template <int TALLY>
LT_DEV void log_append(const WalkParams& P, unsigned idx, typename TallyT<TALLY>::type val, bool has, unsigned long long m,
                       unsigned cnt, unsigned& lg_cur, uint32_t* s_hist)
{
    typedef typename TallyT<TALLY>::type TV;
    if (has) {
        const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        P.log_idx[lg_cur + rank] = idx;
        reinterpret_cast<TV*>(P.log_val)[lg_cur + rank] = val;
        atomicAdd(&s_hist[idx >> P.log_hist_shift], 1u);   // histogram of the first partition pass's bins, kept in LDS
    }
    lg_cur += cnt;
}

template <int TALLY, int ROUTE>
LT_DEV void emit_deposit(const WalkParams& P, unsigned idx, typename TallyT<TALLY>::type val,
                         unsigned& lg_cur, unsigned& lg_end, unsigned& lg_chunk, uint32_t* s_hist)
{
    const bool has = idx != kNoVoxel;
    if constexpr (ROUTE == kRouteAtomic) {
        if (has) tally_add<TALLY>(P.grid, idx, val);
    } else if constexpr (ROUTE == kRouteLog) {
        // The mask of records is the ballot of the integer compare: the v_cmp itself, into a scalar pair.  With room in the chunk
        // an append passes ONE wave-uniform test, of the room.  A wave that has found the log exhausted keeps an empty chunk
        // (lg_cur == lg_end == 0), so the same test sends every later emit of it into the rare block, where the state is looked at:
        // lg_chunk == kLogExhausted is sticky, so an undersized log costs each wave ONE extra returning atomic, not one per emit on
        // 16 shared addresses, and the group counters stay within cap + resident waves -- far from wrapping grp + kLogGroups * c.
        // The rare block is an excursion that comes back in front of the append (a wave that spilled appends nothing: no lane,
        // no record), so the append's path holds no join with it and no flag that says which way the wave came.
        bool rec = has;
        const unsigned long long m = __ballot(has);
        if (m == 0ull) return;
        unsigned cnt = (unsigned)__popcll(m);
        if (__builtin_expect(lg_end - lg_cur < cnt, 0)) {      // once per kLogChunk records -- or the log is exhausted
            if (lg_chunk != kLogExhausted) log_claim(P, lg_cur, lg_end, lg_chunk);
            if (lg_chunk == kLogExhausted) { log_spill<TALLY>(P, idx, val, has, cnt); rec = false; cnt = 0; }
        }
        log_append<TALLY>(P, idx, val, rec, m, cnt, lg_cur, s_hist);
    } else {
        if (P.log_idx == nullptr) {
            if (has) tally_add<TALLY>(P.grid, idx, val);
            return;
        }
        // (the mask from the bool behind the branch: these kernels have no scalar pair to carry it across in)
        const unsigned long long m = __ballot(has);
        if (m == 0ull) return;
        const unsigned cnt = (unsigned)__popcll(m);
        if (lg_chunk != kLogExhausted && lg_end - lg_cur < cnt) log_claim(P, lg_cur, lg_end, lg_chunk);
        if (lg_chunk == kLogExhausted) { log_spill<TALLY>(P, idx, val, has, cnt); return; }
        log_append<TALLY>(P, idx, val, has, m, cnt, lg_cur, s_hist);
    }
}

constexpr unsigned kPacket = 64;  // photon ids taken from the global queue per atomic
#ifndef LT_REFILL_MIN
#define LT_REFILL_MIN 4
#endif
constexpr unsigned kRefillMin = LT_REFILL_MIN;   // dead lanes a wave collects before it refills them
#ifndef LT_QUERY_MIN
#define LT_QUERY_MIN 8
#endif
// mesh walks: lanes a wave collects before it serves their surface queries.  16 was best while every query walked the
// BVH (~1500 instructions per service); with the near-triangle lists (nearest_listed: ~2-4 triangle tests) a service is
// cheap and waiting costs more: C4 f64 walk 37.3 ms at 16, 34.4 at 8, 34.5 at 4, 47.6 at 32 (profiles/r02d_c4_near_lists.log)
constexpr unsigned kQueryMin = LT_QUERY_MIN;
// ... and when the tables live in global memory (GEOM 2): there a service that has to walk the BVH for some lane is a
// chain of dependent loads that costs the wave the same whether 2 lanes or 20 walk, so it pays to wait for many: on the
// 5140-triangle sphere 8 / 16 / 24 / 32 / 48 / 56 / 64 lanes give 4.7 / 5.4 / 6.3 / 7.1 / 8.5 / 8.2 / 5.2e9
// photon-steps/s f64 (profiles/r02e_large_mesh_query_threshold.log).  LT_QUERY_MIN in the environment overrides both.
constexpr unsigned kQueryMinGlobal = 48;
#ifndef LT_QUERY_MAX_AGE
#define LT_QUERY_MAX_AGE 8
#endif
// ... but no lane waits longer than this many wave iterations: where queries are rare (a dense medium around a large mesh)
// the lanes that wait would idle until enough of them have trickled in -- the 5140-triangle sphere in a medium of ten
// times the scattering ran at 4.2e9 photon-steps/s without this bound and at 9.1-9.5e9 with 4 ... 10; C4 gains 1-5 % too
// (profiles/r02e_large_mesh_query_threshold.log)
constexpr unsigned kQueryMaxAge = LT_QUERY_MAX_AGE;
#ifndef LT_MARCH_DRAIN_MIN
#define LT_MARCH_DRAIN_MIN 8
#endif
// walk_kernel_m: queries whose march has ended and that only wait for their queued candidates to be tested; this many
// trigger a drain of a queue that holds less than a full round (LT_QUERY_MIN in the environment overrides)
constexpr unsigned kMarchDrainMin = LT_MARCH_DRAIN_MIN;

// ---------------------------------------------------------------------------
// the walk kernel
// ---------------------------------------------------------------------------
// minimum waves per SIMD the register allocator must leave room for (occupancy is what hides the latency of the
// dependent f64 / transcendental chains once deposition no longer paces the walk)
#ifndef LT_F64_WAVES
#define LT_F64_WAVES 4        // f64 mesh walks: ~80 B of scratch per lane at 128 VGPRs, still 6 % faster than 3 waves (C4)
#endif
#ifndef LT_F64_GLOBAL_WAVES
#define LT_F64_GLOBAL_WAVES 3 // f64 walks of meshes beyond LDS (grid march): the DDA state on top of the photon's does not fit 128 VGPRs
#endif
#ifndef LT_F64_SLAB_WAVES
#define LT_F64_SLAB_WAVES 4   // f64 slab walks fit 128 VGPRs without scratch since the polynomial constants live in SGPRs
#endif
#ifndef LT_F32_WAVES
#define LT_F32_WAVES 5
#endif
// where the walk keeps the grid's origin / inverse voxel size / dimensions (lt_walk_kernel.inc, LT_INV_MODE), chosen per kernel
// from same-box A/B runs (profiles/r04c_ab_modes.log):
//   slab kernels   1, pinned VGPRs: f64 127 VGPRs, the fewest VALU instructions (C2 walk 26.3 ms against 26.9 converted in
//                  the kernel, 27.0 as scalar arguments, 27.2 from LDS) -- and the leaner builds (109-110 VGPRs) made the log
//                  reduction beside a half-occupancy walk much slower (two lanes: 40.6-42.5 ms against 37.5-37.9)
//   LDS-mesh       2, LDS: the Cornell kernel needs its 128 VGPRs for the photon and the held step; no scratch (60 B pinned),
//                  C4 walk 28.4 ms against 31.7 pinned and 33.5 in round 3
//   march kernel   2, LDS: teapot / cow / pumpkin 19.0 / 18.9 / 17.8e9 f64 steps/s against 17.8 / 17.6 / 16.9 as scalar arguments
//                  (156 VGPRs without scratch, but the scalar file overflows into v_readlane restores) and 18.1 / 18.0 / 17.1
//                  pinned (profiles/r04d_march_modes.log); 154 VGPRs + 36 B of scratch
#ifndef LT_INV_MODE_SLAB
#define LT_INV_MODE_SLAB 1
#endif
#ifndef LT_INV_MODE_MESH
#define LT_INV_MODE_MESH 2
#endif
#ifndef LT_INV_MODE_MARCH
#define LT_INV_MODE_MARCH 2
#endif
// the two optional forms of the f64 slab walk's step diet, for same-box A/B builds (profiles/r12a_step_diet_ab.log):
//   LT_DIET_SIGN32    the in-grid test's sign test on the coordinates' high words alone
//   LT_DIET_MASKSUM   deposit and energy sums under the in-grid lane mask instead of selects
#ifndef LT_DIET_SIGN32
#define LT_DIET_SIGN32 1
#endif
#ifndef LT_DIET_MASKSUM
#define LT_DIET_MASKSUM 1
#endif
#define LT_INV_MODE LT_INV_MODE_SLAB
#define LT_WALK_NAME walk_kernel
#define LT_WALK_BATCH 0
#include "lt_walk_kernel.inc"
#undef LT_WALK_NAME
#undef LT_WALK_BATCH
#undef LT_INV_MODE
#define LT_INV_MODE LT_INV_MODE_MESH
#define LT_WALK_NAME walk_kernel_q
#define LT_WALK_BATCH 1
#include "lt_walk_kernel.inc"
#undef LT_WALK_NAME
#undef LT_WALK_BATCH
#undef LT_INV_MODE
#define LT_INV_MODE LT_INV_MODE_MARCH
#define LT_WALK_NAME walk_kernel_m
#define LT_WALK_BATCH 2
#include "lt_walk_kernel.inc"
#undef LT_WALK_NAME
#undef LT_WALK_BATCH
#undef LT_INV_MODE

// ---------------------------------------------------------------------------
// variant dispatch
// ---------------------------------------------------------------------------
typedef void (*WalkFn)(const WalkParams);

// CAPTURE (light sub-path vertices, f4) is a compile-time variant: the capture code costs the plain walk registers
// even behind a never-taken branch (36-84 B of scratch per lane, walk 29.7 -> 34.6 ms when it was a run-time test).
// Captures run the f64 walk with the XORWOW generator.
// slabs: walk_kernel, a build per deposit route (Variant::route) -- of what lt_launch can ask for: the log carries neither
// table-RNG walks nor captures nor the diagnostic build without a tally; the bulk kernel (PHASE 1) fills a log, the tail kernel
// (PHASE 2) deposits with atomics.  Anything else is no kernel, and a launch of it an error.
template <typename R, bool TABLE, bool CAPTURE, int PHASE, int ROUTE>
static WalkFn pick_slab(int tally)
{
    constexpr bool kBuilt = (ROUTE == kRouteLog ? !TABLE && !CAPTURE && PHASE != 2 : PHASE != 1) && (PHASE == 0 || (!TABLE && !CAPTURE));
    if constexpr (kBuilt) {
        switch (tally) {
        case LT_TALLY_F32:
            if constexpr (TABLE) return nullptr;
            else return walk_kernel<R, 0, TABLE, LT_TALLY_F32, CAPTURE, PHASE, ROUTE>;
        case LT_TALLY_F64: return walk_kernel<R, 0, TABLE, LT_TALLY_F64, CAPTURE, PHASE, ROUTE>;
        case LT_TALLY_U64FX: return walk_kernel<R, 0, TABLE, LT_TALLY_U64FX, CAPTURE, PHASE, ROUTE>;
        case LT_TALLY_NONE:
            if constexpr (!TABLE && !CAPTURE && PHASE == 0 && ROUTE == kRouteAtomic) return walk_kernel<R, 0, false, LT_TALLY_NONE, false, 0, kRouteAtomic>;
            else return nullptr;
        }
    }
    return nullptr;
}

// meshes: walk_kernel_q (the same body with batched BVH queries, lt_walk_kernel.inc)
template <typename R, int GEOM, bool TABLE, bool CAPTURE>
static WalkFn pick_tally(int tally)
{
    switch (tally) {
    case LT_TALLY_F32:
        if constexpr (TABLE) return nullptr;
        else return walk_kernel_q<R, GEOM, TABLE, LT_TALLY_F32, CAPTURE>;
    case LT_TALLY_F64: return walk_kernel_q<R, GEOM, TABLE, LT_TALLY_F64, CAPTURE>;
    case LT_TALLY_U64FX: return walk_kernel_q<R, GEOM, TABLE, LT_TALLY_U64FX, CAPTURE>;
    }
    return nullptr;
}

// meshes beyond LDS with a march grid (Variant::mesh 3): walk_kernel_m, tables in global memory (GEOM 2)
template <typename R, bool CAPTURE>
static WalkFn pick_march(int tally)
{
    switch (tally) {
    case LT_TALLY_F32: return walk_kernel_m<R, 2, false, LT_TALLY_F32, CAPTURE>;
    case LT_TALLY_F64: return walk_kernel_m<R, 2, false, LT_TALLY_F64, CAPTURE>;
    case LT_TALLY_U64FX: return walk_kernel_m<R, 2, false, LT_TALLY_U64FX, CAPTURE>;
    }
    return nullptr;
}

template <typename R, bool TABLE, bool CAPTURE>
static WalkFn pick_geom(const Variant& v)
{
    if (v.mesh == 3) { if constexpr (!TABLE) return pick_march<R, CAPTURE>(v.tally); else return nullptr; }
    if (v.mesh == 0)
        return v.route == kRouteLog ? pick_slab<R, TABLE, CAPTURE, 0, kRouteLog>(v.tally) : pick_slab<R, TABLE, CAPTURE, 0, kRouteAtomic>(v.tally);
    if (v.mesh == 1) return pick_tally<R, 1, TABLE, CAPTURE>(v.tally);
    if constexpr (!TABLE) return pick_tally<R, 2, TABLE, CAPTURE>(v.tally); else return nullptr;
}

// the walk through a mesh in LDS in two kernels (Variant::phase 1 / 2, lt_walk_kernel.inc "Tail split"): XORWOW, no capture
template <typename R, int PHASE>
static WalkFn pick_phase_q(int tally)
{
    switch (tally) {
    case LT_TALLY_F32: return walk_kernel_q<R, 1, false, LT_TALLY_F32, false, PHASE>;
    case LT_TALLY_F64: return walk_kernel_q<R, 1, false, LT_TALLY_F64, false, PHASE>;
    case LT_TALLY_U64FX: return walk_kernel_q<R, 1, false, LT_TALLY_U64FX, false, PHASE>;
    }
    return nullptr;
}

static WalkFn pick(const Variant& v)
{
    if (v.route != kRouteAtomic && v.route != kRouteLog) return nullptr;
    if (v.phase) {
        if (v.mesh > 1 || v.table || v.capture) return nullptr;
        if (v.mesh == 1) {
            if (v.phase == 1) return v.f32 ? pick_phase_q<float, 1>(v.tally) : pick_phase_q<double, 1>(v.tally);
            return v.f32 ? pick_phase_q<float, 2>(v.tally) : pick_phase_q<double, 2>(v.tally);
        }
        if (v.phase == 1) {
            if (v.route != kRouteLog) return nullptr;
            return v.f32 ? pick_slab<float, false, false, 1, kRouteLog>(v.tally) : pick_slab<double, false, false, 1, kRouteLog>(v.tally);
        }
        if (v.route != kRouteAtomic) return nullptr;
        return v.f32 ? pick_slab<float, false, false, 2, kRouteAtomic>(v.tally) : pick_slab<double, false, false, 2, kRouteAtomic>(v.tally);
    }
    if (v.capture) return (v.f32 || v.table) ? nullptr : pick_geom<double, false, true>(v);
    if (v.f32) return v.table ? nullptr : pick_geom<float, false, false>(v);
    return v.table ? pick_geom<double, true, false>(v) : pick_geom<double, false, false>(v);
}

size_t walk_lds_bytes(const Variant& v, int n_media, int n_layers, int n_tris, int n_nodes, unsigned n_hist)
{
    if (v.mesh) n_layers = 0;
    if (v.mesh != 1) { n_tris = 0; n_nodes = 0; }
    // walk_kernel_m (mesh 3): the march's per-wave scratch (rays, best hits, candidate queue), four waves per workgroup.  The
    // plain global-memory kernel (mesh 2: no march grid / LT_NO_MARCH) never touches it and keeps its LDS free
    return v.f32 ? LdsLayout<float>(n_media, n_layers, n_tris, n_nodes, n_hist, v.mesh == 3 ? 4 * sizeof(MarchWave<float>) : 0).total
                 : LdsLayout<double>(n_media, n_layers, n_tris, n_nodes, n_hist, v.mesh == 3 ? 4 * sizeof(MarchWave<double>) : 0).total;
}

int walk_max_blocks_per_cu(const Variant& v, int threads, size_t lds_bytes)
{
    WalkFn fn = pick(v);
    if (!fn) return 0;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(fn), threads, lds_bytes) != hipSuccess)
        return 0;
    return nb;
}

hipError_t launch_walk(const WalkParams& Pin, const Variant& vin, const LaunchCfg& cfg, hipStream_t s)
{
    Variant v = vin;
    v.route = Pin.log_idx ? kRouteLog : kRouteAtomic;      // the one place a launch's route is decided: the kernel that runs is the build for these parameters
    WalkFn fn = pick(v);
    if (!fn) return hipErrorInvalidValue;
    WalkParams P = Pin;
    if (v.mesh) P.n_layers = 0; else { P.n_tris = 0; P.n_nodes = 0; }
    if (cfg.lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)cfg.lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fn, dim3(cfg.blocks), dim3(cfg.threads), cfg.lds_bytes, s, P);
    return hipGetLastError();
}

}  // namespace ltk
