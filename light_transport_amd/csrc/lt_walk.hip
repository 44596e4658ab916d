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
    __host__ __device__ LdsLayout(int n_media, int n_layers, int n_tris, int n_nodes, unsigned n_hist = 0, size_t march_bytes = 0)
    {
        auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
        size_t o = 0;
        off_cnt = o;   o = al(o + 8 * sizeof(double));
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

// One deposit record per lane (or none) leaves the lane's run-length accumulator.  Atomic mode: a no-return
// global atomic.  Log mode: the wave's records are compacted by ballot rank and appended, coalesced, to the wave's
// current log chunk (SoA: voxel index, value); a chunk is claimed with one returning atomic per kLogChunk records.
// If the log is exhausted the wave falls back to atomics, so a too-small log costs speed, never correctness.
// A lane without a record passes idx == kNoVoxel (its val is then not read).  IDX_MASK (the slab walks): the wave's mask of
// records is the ballot of that integer compare, taken in front of the tally-mode branch: there it IS the compare's result (one
// v_cmp into a scalar pair).  Taken from the bool behind the branch (the mesh walks, which have no scalar pair to carry it in) it
// costs a round trip through a VGPR (v_cndmask 0,1 + v_cmp_ne) in every wave-step.
constexpr unsigned kLogExhausted = 0xfffffffeu;   // lg_chunk: this wave has found the log full (0xffffffff: no chunk claimed yet)
constexpr unsigned kNoVoxel = 0xffffffffu;        // idx: no record
template <int TALLY, bool IDX_MASK>
LT_DEV void emit_deposit(const WalkParams& P, unsigned idx, typename TallyT<TALLY>::type val,
                         unsigned& lg_cur, unsigned& lg_end, unsigned& lg_chunk, uint32_t* s_hist)
{
    typedef typename TallyT<TALLY>::type TV;
    const bool has = idx != kNoVoxel;
    unsigned long long m = 0;
    if constexpr (IDX_MASK) m = __ballot(has);
    if (P.log_idx == nullptr) {
        if (has) tally_add<TALLY>(P.grid, idx, val);
        return;
    }
    if constexpr (!IDX_MASK) m = __ballot(has);
    if (m == 0ull) return;
    const unsigned cnt = (unsigned)__popcll(m);
    // (a wave that has found the log exhausted does not ask again: lg_chunk == kLogExhausted is sticky, so an undersized log
    // costs each wave ONE extra returning atomic, not one per emit on 16 shared addresses, and the group counters stay
    // within cap + resident waves -- far from wrapping grp + kLogGroups * c)
    if (lg_chunk != kLogExhausted && lg_end - lg_cur < cnt) {
        const int lane = threadIdx.x & 63;
        const unsigned grp = blockIdx.x & (kLogGroups - 1);
        if (lg_chunk < kLogExhausted && lane == 0) P.log_fill[lg_chunk] = lg_cur - lg_chunk * kLogChunk;
        unsigned c = 0;
        if (lane == 0) c = __hip_atomic_fetch_add(P.log_next + grp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        c = grp + kLogGroups * __builtin_amdgcn_readfirstlane(c);     // the group's own chunks: see kLogGroups
        if (c < P.log_cap_chunks) { lg_chunk = c; lg_cur = c * kLogChunk; lg_end = lg_cur + kLogChunk; }
        else { lg_chunk = kLogExhausted; lg_cur = lg_end = 0; }
    }
    if (lg_chunk == kLogExhausted) {  // log exhausted: back to the linear voxel index and a global atomic
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
        return;
    }
    if (has) {
        const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        P.log_idx[lg_cur + rank] = idx;
        reinterpret_cast<TV*>(P.log_val)[lg_cur + rank] = val;
        atomicAdd(&s_hist[idx >> P.log_hist_shift], 1u);   // histogram of the first partition pass's bins, kept in LDS
    }
    lg_cur += cnt;
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
template <typename R, int GEOM, bool TABLE, bool CAPTURE>
static WalkFn pick_tally(int tally)
{
    switch (tally) {
    // slabs: walk_kernel; meshes: walk_kernel_q (the same body with batched BVH queries, lt_walk_kernel.inc)
    case LT_TALLY_F32:
        if constexpr (TABLE) return nullptr;
        else if constexpr (GEOM == 0) return walk_kernel<R, GEOM, TABLE, LT_TALLY_F32, CAPTURE>;
        else return walk_kernel_q<R, GEOM, TABLE, LT_TALLY_F32, CAPTURE>;
    case LT_TALLY_F64:
        if constexpr (GEOM == 0) return walk_kernel<R, GEOM, TABLE, LT_TALLY_F64, CAPTURE>;
        else return walk_kernel_q<R, GEOM, TABLE, LT_TALLY_F64, CAPTURE>;
    case LT_TALLY_U64FX:
        if constexpr (GEOM == 0) return walk_kernel<R, GEOM, TABLE, LT_TALLY_U64FX, CAPTURE>;
        else return walk_kernel_q<R, GEOM, TABLE, LT_TALLY_U64FX, CAPTURE>;
    case LT_TALLY_NONE:
        if constexpr (!TABLE && GEOM == 0 && !CAPTURE) return walk_kernel<R, GEOM, TABLE, LT_TALLY_NONE, false>; else return nullptr;
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
    if (v.mesh == 0) return pick_tally<R, 0, TABLE, CAPTURE>(v.tally);
    if (v.mesh == 1) return pick_tally<R, 1, TABLE, CAPTURE>(v.tally);
    if constexpr (!TABLE) return pick_tally<R, 2, TABLE, CAPTURE>(v.tally); else return nullptr;
}

// slab walks in two kernels (Variant::phase 1 / 2, lt_walk_kernel.inc "Tail split"): XORWOW, no capture
template <typename R, int PHASE>
static WalkFn pick_phase(int tally)
{
    switch (tally) {
    case LT_TALLY_F32: return walk_kernel<R, 0, false, LT_TALLY_F32, false, PHASE>;
    case LT_TALLY_F64: return walk_kernel<R, 0, false, LT_TALLY_F64, false, PHASE>;
    case LT_TALLY_U64FX: return walk_kernel<R, 0, false, LT_TALLY_U64FX, false, PHASE>;
    }
    return nullptr;
}

// ... and the walk through a mesh in LDS (Variant::mesh 1)
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
    if (v.phase) {
        if (v.mesh > 1 || v.table || v.capture) return nullptr;
        if (v.mesh == 1) {
            if (v.phase == 1) return v.f32 ? pick_phase_q<float, 1>(v.tally) : pick_phase_q<double, 1>(v.tally);
            return v.f32 ? pick_phase_q<float, 2>(v.tally) : pick_phase_q<double, 2>(v.tally);
        }
        if (v.phase == 1) return v.f32 ? pick_phase<float, 1>(v.tally) : pick_phase<double, 1>(v.tally);
        return v.f32 ? pick_phase<float, 2>(v.tally) : pick_phase<double, 2>(v.tally);
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

hipError_t launch_walk(const WalkParams& Pin, const Variant& v, const LaunchCfg& cfg, hipStream_t s)
{
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
