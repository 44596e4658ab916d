// lt_walk_kernel.inc -- body of the walk kernel, included three times by lt_walk.hip:
//   LT_WALK_BATCH 0 -> walk_kernel     (layered slabs): prepare and complete a step back to back;
//   LT_WALK_BATCH 1 -> walk_kernel_q   (meshes): lanes that need a BVH query hold their prepared step until enough
//                                       of them have gathered (see the comment at the step).
//   LT_WALK_BATCH 2 -> walk_kernel_m   (meshes beyond LDS with a march grid): a surface query is marched through the
//                                       candidate grid ONE CELL PER WAVE ITERATION beside the other lanes' steps, its
//                                       candidates are tested by the whole wave (march_round / march_drain).
// Everything outside the step's head is the same text.
// Tail split (walk_kernel and walk_kernel_q, PHASE 1 / 2; PHASE 0 is the whole walk in one kernel).  The last ~3 ms of a 1e7-photon walk
// are a DRAIN: the queue is empty and lone waves finish the few photons that keep winning the roulette (~2000 steps where
// the mean is 283), while the partition of the batch's deposit log cannot start before the kernel ends.  PHASE 1 ends early:
// a wave that can get no more photons and has at most kDumpMaxLanes alive flushes its pending deposits and writes those
// photons' complete state (SurvD) to a pool; the host then starts the log reduction on the lane's stream and, beside it on
// another stream, PHASE 2, whose waves take 64 pool entries each and walk them to the end with atomic deposits.  A photon's
// trajectory depends on its own state only, so results are unchanged (u64 tally bit for bit).
// the record of medium i in LDS by a 24-bit multiply (v_mul_u32_u24, full rate; plain indexing compiles to the quarter-rate v_mul_lo_u32)
#ifndef LT_MED
#define LT_MED(i) reinterpret_cast<const MedD<R>*>(reinterpret_cast<const unsigned char*>(s_med) + __umul24((unsigned)(i), (unsigned)sizeof(MedD<R>)))
#define LT_LAY(i) reinterpret_cast<const LayD<R>*>(reinterpret_cast<const unsigned char*>(s_lay) + __umul24((unsigned)(i), (unsigned)sizeof(LayD<R>)))
#endif
// measurement builds of the slab walk (see its step): 1 = read the layer record's interaction fields / the math-table cells
// where they are used instead of at the top of the step (profiles/r05a_layer_record_ab.log: both early reads pay)
#ifndef LT_LAY_LATE
#define LT_LAY_LATE 0
#endif
#ifndef LT_TAB_LATE
#define LT_TAB_LATE 0
#endif
// what the interaction block (the same text for every kernel) takes from the medium: the slab kernel holds the fields of its
// layer record (LayD, read at the top of the step), the mesh kernels read their medium's record (MedD) where they use it
#if LT_WALK_BATCH == 0
#define LT_STEP_Y(held, field) (kLayEarly ? held : Yp->field)
#define LT_STEP_ABSORB LT_STEP_Y(absorb, absorb)
#define LT_STEP_DEP LT_STEP_Y(dep, dep)
#define LT_STEP_HG(xi) hg_sample_walk(xi, LT_STEP_Y(hg_2g, two_g), LT_STEP_Y(hg_1mg, one_m_g), LT_STEP_Y(hg_1mg2, one_m_g2), LT_STEP_Y(hg_1pg2, one_p_g2), LT_STEP_Y(hg_i2g, inv_2g))
#define LT_STEP_G (LT_MED(s_lm[cur])->g)      // (vertex capture only: the phase function's density)
#else
#define LT_STEP_ABSORB Mp->absorb
#define LT_STEP_DEP Mp->dep
#define LT_STEP_HG(xi) hg_sample_walk(xi, Mp)
#define LT_STEP_G (Mp->g)
#endif
#if LT_WALK_BATCH == 0
template <typename R, int GEOM, bool TABLE, int TALLY, bool CAPTURE, int PHASE, int ROUTE>      // ROUTE: kRouteAtomic / kRouteLog (emit_deposit)
#elif LT_WALK_BATCH == 1
template <typename R, int GEOM, bool TABLE, int TALLY, bool CAPTURE, int PHASE = 0>
#else
template <typename R, int GEOM, bool TABLE, int TALLY, bool CAPTURE>
#endif
__global__ void __launch_bounds__(256, (sizeof(R) == 8 ? (GEOM == 0 ? LT_F64_SLAB_WAVES : (GEOM == 2 ? LT_F64_GLOBAL_WAVES : LT_F64_WAVES)) : (GEOM == 0 ? LT_F32_WAVES : 4))) LT_WALK_NAME(const WalkParams P)
{
    constexpr bool MESH = GEOM != 0;
    // Wave bookkeeping off the vector pipe (profiles/r07a_walk_bookkeeping.log).  kSlabForm, every slab walk: the 32-bit packet
    // cursor, the refill count as a 32-bit scalar, the deposit mask taken on the index compare (emit_deposit), the tile index by
    // mad_u24.  kLean: the two forms that lengthen a value's life -- `need` kept to the loop's exit, f_val without a default.  The
    // tail kernel (PHASE 2) takes them too: 84-88 VGPRs where it had 84-86, the same five waves per SIMD.  The vertex capture does
    // not (it spilled 20-28 B), nor do the mesh walks take any of these forms: they sit at their register limits, and the log has
    // the register and scratch figures of the mesh kernels built with all of them and with the 32-bit cursor alone.
    constexpr bool kSlabForm = LT_WALK_BATCH == 0;
    constexpr bool kLean = kSlabForm && !CAPTURE;
    // The step diet of DESIGN.md section 5 (dimensions from LDS, one product for the deposit, masked sums, the scalar step count, the
    // interface decision as a mask): the f64 slab walks.  The f32 slab walks keep their text: their only yardstick is that every f32
    // build rounds alike (tests/test_walk_invariances.py), and with these forms the bulk and tail kernels no longer did.
    constexpr bool kDiet = kSlabForm && sizeof(R) == 8;
    constexpr bool kMaskSum = kDiet && kLean && LT_DIET_MASKSUM != 0;      // (and LT_DIET_SIGN32: the two optional forms, lt_walk.hip)
#if LT_WALK_BATCH == 2
    constexpr int PHASE = 0;
#endif
    // Where the deposit records go.  Slab walks: fixed per build -- the log build computes the tiled voxel index alone and appends,
    // the atomic build has no tile index, no log cursor and no histogram.  The bulk kernel (PHASE 1) exists to fill a log, the
    // tail kernel (PHASE 2) deposits with atomics beside that log's reduction.  Mesh walks: P.log_idx, asked where it matters.
#if LT_WALK_BATCH == 0
    constexpr int kRoute = ROUTE;
#define LT_HAS_LOG (ROUTE == kRouteLog)
    static_assert(ROUTE == kRouteAtomic || ROUTE == kRouteLog, "walk_kernel is built per deposit route");
    static_assert((PHASE != 1 || ROUTE == kRouteLog) && (PHASE != 2 || ROUTE == kRouteAtomic), "bulk kernel: log; tail kernel: atomics");
#else
    constexpr int kRoute = kRouteRuntime;
#define LT_HAS_LOG P.log_idx
#endif
#if LT_WALK_PRIO
    // The walk is bound by VALU issue; the log reductions that share its CUs (another job's partition and tile reduce) are not.
    // Raised wave priority lets the walk's waves issue first and the co-runners fill what is left.
    __builtin_amdgcn_s_setprio(LT_WALK_PRIO);
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    // GEOM 2: the mesh is too large for LDS -> triangles and nodes are read from global memory (they are
    // read-only and shared by every wave, so they live in the XCD L2s / Infinity Cache after first touch)
    const LdsLayout<R> L(P.n_media, P.n_layers, GEOM == 1 ? P.n_tris : 0, GEOM == 1 ? P.n_nodes : 0,
                         LT_HAS_LOG ? P.log_n_hist : 0u, LT_WALK_BATCH == 2 ? 4 * sizeof(MarchWave<R>) : 0);
    uint32_t* s_hist = reinterpret_cast<uint32_t*>(lds_raw + L.off_hist);   // log mode: records per partition bin (<= 4 KiB)
    if (LT_HAS_LOG) for (unsigned t = threadIdx.x; t < P.log_n_hist; t += blockDim.x) s_hist[t] = 0;
    double* s_cnt = reinterpret_cast<double*>(lds_raw + L.off_cnt);
    const MedD<R>* s_med = reinterpret_cast<const MedD<R>*>(lds_raw + L.off_media);
    const R* s_zb = reinterpret_cast<const R*>(lds_raw + L.off_zb);
    const int32_t* s_lm = reinterpret_cast<const int32_t*>(lds_raw + L.off_lm);
    // slab walks: the per-layer step records.  kLean builds that read the record at the top of the step hold the table's offset in a
    // VGPR (one of the two the per-lane step count left): as a scalar it was moved into one in every step -- the record's address is
    // a 24-bit multiply-add whose other factor is a scalar already -- and in the bulk kernel it was a spilled scalar besides.
    unsigned lay_off = (unsigned)L.off_lay;
    if constexpr (kDiet && !CAPTURE && PHASE != 2) asm volatile("" : "+v"(lay_off));
    [[maybe_unused]] const LayD<R>* s_lay = reinterpret_cast<const LayD<R>*>(lds_raw + lay_off);
    const IfD<R>* s_if = reinterpret_cast<const IfD<R>*>(lds_raw + L.off_if);
    const TriD<R>* s_tris = GEOM == 2 ? reinterpret_cast<const TriD<R>*>(P.tris)
                                      : reinterpret_cast<const TriD<R>*>(lds_raw + L.off_tris);
    const NodeD<R>* s_nodes = GEOM == 2 ? reinterpret_cast<const NodeD<R>*>(P.nodes)
                                        : reinterpret_cast<const NodeD<R>*>(lds_raw + L.off_nodes);

    // front-to-back link tables of the BVH (null: a mesh of more than 32767 nodes -- its rare BVH searches go in storage order)
    const int16_t* s_links = !MESH || !P.links ? nullptr
                             : (GEOM == 1 ? reinterpret_cast<const int16_t*>(lds_raw + L.off_links) : P.links);
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0.0;
    R* s_frame = reinterpret_cast<R*>(lds_raw + L.off_frame);
    if (threadIdx.x == 64 % blockDim.x && P.src_type == LT_SRC_COSINE_QUAD) {      // create_orthonormal_system of the source normal, once
        const R nrm[3] = {(R)P.src_dir[0], (R)P.src_dir[1], (R)P.src_dir[2]};
        R v2[3], v3[3];
        onb(nrm, v2, v3);
#pragma unroll
        for (int k = 0; k < 3; k++) { s_frame[k] = v2[k]; s_frame[3 + k] = v3[k]; }
    }
    // Slab walks: the grid's dimensions for the in-grid test, and the count of capped photons (LdsLayout::kSlabDim / kSlabCap).
    // As kernel arguments the three dimensions were spilled scalars in the log build, restored by four v_readlane in every step.
    constexpr bool kDimLds = kDiet && LT_INV_MODE != 2;
    // the photon-step count on the scalar unit (see `steps_w` at the step); the vertex capture keeps its per-lane counter
    constexpr bool kStepsScalar = kLean && kDimLds;
    if constexpr (kDimLds) {
        typedef LdsLayout<R> LL;
        static_assert(LL::kSlabDim % 16 == 0 && LL::kSlabDim >= LL::kFrame + 6 * sizeof(R) && LL::kSlabDim + 16 <= ((LL::kFrame + 15 * sizeof(R) + 15) & ~(size_t)15),
                      "the dimensions: behind the source frame, inside the frame block");
        static_assert(LL::kSlabCap % 8 == 0 && LL::kSlabCap >= LL::kFrame + 6 * sizeof(R) && LL::kSlabCap + 8 <= LL::kFrame + 15 * sizeof(R) &&
                      (LL::kSlabCap + 8 <= LL::kSlabDim || LL::kSlabCap >= LL::kSlabDim + 16), "the capped count: likewise, clear of the dimensions");
        if (threadIdx.x == 128 % blockDim.x) {
            unsigned* d = reinterpret_cast<unsigned*>(lds_raw + LdsLayout<R>::kSlabDim);
            d[0] = (unsigned)P.nx; d[1] = (unsigned)P.ny; d[2] = (unsigned)P.nz; d[3] = 0u;
            *reinterpret_cast<unsigned long long*>(lds_raw + LdsLayout<R>::kSlabCap) = 0ull;
        }
    }
#if LT_INV_MODE == 2
    const R* s_inv = s_frame + 6;       // grid origin, inverse voxel size, dimensions (see LT_INV_MODE below)
    if (threadIdx.x == 128 % blockDim.x) {
#pragma unroll
        for (int k = 0; k < 3; k++) { s_frame[6 + k] = LT_PV(origin, k); s_frame[9 + k] = LT_PV(inv_voxel, k); s_frame[12 + k] = LT_PV(fdim, k); }
    }
#endif
    const double* s_math = reinterpret_cast<const double*>(lds_raw + L.off_math);      // f64: -ln / sin-cos tables (neg_log_tab, sincos_turn_tab)
    if constexpr (sizeof(R) == 8) lds_copy(lds_raw + L.off_math, kWalkMathTab, kWalkMathTabBytes);
    lds_copy(lds_raw + L.off_media, P.media, (size_t)P.n_media * sizeof(MedD<R>));
    if constexpr (!MESH) {
        lds_copy(lds_raw + L.off_zb, P.zb, (size_t)(P.n_layers + 1) * sizeof(R));
        lds_copy(lds_raw + L.off_lm, P.layer_medium, (size_t)P.n_layers * sizeof(int32_t));
        lds_copy(lds_raw + L.off_if, P.ifaces, (size_t)(P.n_layers + 1) * sizeof(IfD<R>));
        lds_copy(lds_raw + L.off_lay, P.layers, (size_t)P.n_layers * sizeof(LayD<R>));
    } else if constexpr (GEOM == 1) {
        lds_copy(lds_raw + L.off_tris, P.tris, (size_t)P.n_tris * sizeof(TriD<R>));
        lds_copy(lds_raw + L.off_nodes, P.nodes, (size_t)P.n_nodes * sizeof(NodeD<R>));
        if (P.links) lds_copy(lds_raw + L.off_links, P.links, (size_t)P.n_nodes * 16 * sizeof(int16_t));
    }
    __syncthreads();

    const R eps = (R)1e-6;  // EPSILON, S/constants.py:12
    const R inf = Mx<R>::inf();
    const int lane = threadIdx.x & 63;

    // per-lane photon state
    bool alive = false;
    R px = 0, py = 0, pz = 0, ux = 0, uy = 0, uz = 1, w = 0, sleft = 0;
    int cur = 0;
    unsigned step = 0, max_steps = P.max_steps, nv = 0;
    unsigned long long pid = 0, grp = 0;
    rocrand_state_xorwow rng;
    // per-lane accumulators of the frequent events
    double acc_abs = 0.0, acc_lost = 0.0;
    unsigned long long acc_steps = 0;
    // kStepsScalar: the photon-steps of the whole wave instead, counted on the scalar unit.  The lanes that take a step in an
    // iteration are the live ones less those that meet the step cap, and a count inside the step's branch would be a per-lane value
    // again (the lanes outside the branch keep the old one), so it is taken where the wave is whole: the live lanes at the top of
    // the step (the bits `need` leaves clear: s_andn2 / s_bcnt1 / s_add / s_addc), less the photons the bulk kernel hands over
    // behind that (in its wave-uniform block), less the capped ones (counted in LDS where they are capped, taken off once per
    // workgroup at the end).  All integers: the total is exact.
    [[maybe_unused]] unsigned long long steps_w = 0;
    // run-length accumulation: consecutive deposits into the same voxel (a third of all steps when the
    // voxel is one mean free path wide) are summed in registers and sent as ONE atomic request
    typedef typename TallyT<TALLY>::type TV;
    unsigned pend_idx = kNoVoxel;
    TV pend_val = 0;
    // wave-level deposit-log cursor (log mode): records [lg_cur, lg_end) of chunk lg_chunk are free
    unsigned lg_cur = 0, lg_end = 0, lg_chunk = kNoVoxel;
    // wave-level packet of photon ids [pk_base + pk_next, pk_base + pk_end).  Slab walks: a packet is at most kPacket ids, so
    // the cursor is a pair of 32-bit offsets that the scalar unit compares (it has no ordered 64-bit compare: each would be a
    // v_mov_b64 + v_cmp_*_u64 on the vector pipe, in every wave-step that has a dead lane), and only the base is 64 bits wide.
    // Mesh walks: the offsets are the ids themselves and the base stays 0 (the 32-bit form costs those kernels a register).
    typedef typename std::conditional<kSlabForm, unsigned, unsigned long long>::type pk_t;
    unsigned long long pk_base = 0;
    pk_t pk_next = 0, pk_end = 0;
    bool q_done = false;
    bool dumped = false;      // PHASE 1: this wave has handed its last photons to the pool
#if LT_WALK_BATCH
    // mesh walks: a prepared step waiting for its BVH query (see the step's stage B)
    bool q_pend = false;
#if LT_WALK_BATCH == 1
    // (its free path is sleft / mu_t again when the step resumes: neither changes while it waits)
    typename HeldU<R, TABLE>::type q_u1 = 0, q_u2 = 0, q_u3 = 0;
#endif
#if LT_WALK_BATCH == 2
    // (its prepared step -- free path and decision uniforms -- waits in LDS, MarchWave::held: the kernel has no registers to spare)
    // ... or marching through the candidate grid: q_tc = how far along its hop the query has got, q_march = still
    // visiting cells, q_dirty = candidates of it wait in the queue, q_bvh = the grid cannot answer it
    R q_tc = 0;
    bool q_march = false, q_dirty = false, q_bvh = false;
    unsigned mq_n = 0;        // items in the wave's candidate queue (wave-uniform)
    MarchWave<R>* const mw = reinterpret_cast<MarchWave<R>*>(lds_raw + L.off_march) + (threadIdx.x >> 6);
#endif
#if defined(LT_DIAG_MESH)   /* instrumentation build: where do the wave iterations of a mesh walk go? (workgroup 0, wave 0 prints) */
    unsigned long long dg_iter = 0, dg_alive = 0, dg_prep = 0, dg_wait = 0, dg_trav_it = 0, dg_trav = 0, dg_go = 0, dg_bnd_it = 0, dg_bnd = 0,
                       dg_int_it = 0, dg_int = 0, dg_refill_it = 0, dg_refill = 0, dg_bvh_it = 0, dg_bvh = 0, dg_l4_it = 0, dg_l4 = 0;
    unsigned long long dg_clk_srv = 0, dg_clk_bnd = 0, dg_clk_all = clock64();
    unsigned long long dgm_clk[4] = {0, 0, 0, 0};      // walk_kernel_m: cycles in prepare / march round / drain / resolve
#endif
#endif

#if LT_WALK_BATCH == 1
    const unsigned query_min = P.query_min ? P.query_min : (GEOM == 2 ? kQueryMinGlobal : kQueryMin);
    unsigned q_age = 0;       // wave iterations since some lane began to wait for a service (wave-uniform)
#elif LT_WALK_BATCH == 2
    const unsigned drain_min = P.query_min ? P.query_min : kMarchDrainMin;
#endif
    // The grid's origin, inverse voxel size and dimensions are read by every photon-step.  They arrive as kernel arguments in
    // walk precision (scalar registers).  Left there they -- with the kernel's pointers, queue and log cursors and wave masks --
    // overflow the scalar file, and the allocator spills scalars into VGPR lanes and restores them with v_readlane (a VALU
    // instruction each) in every iteration: ~40 per photon-step measured in the ISA of the f64 slab kernel.  Converted inside
    // the kernel (round 3) they sat in VGPRs through the whole loop (125 VGPRs; the mesh kernels spilled 60 B of them to scratch).
    // LT_INV_MODE: 0 scalar arguments, 1 copied once into VGPRs that an empty asm pins, 2 kept in LDS and read where used.
#if LT_INV_MODE == 2
#define gx0 s_inv[0]
#define gy0 s_inv[1]
#define gz0 s_inv[2]
#define ivx s_inv[3]
#define ivy s_inv[4]
#define ivz s_inv[5]
#define fnx s_inv[6]
#define fny s_inv[7]
#define fnz s_inv[8]
#else
    R gx0 = LT_PV(origin, 0), gy0 = LT_PV(origin, 1), gz0 = LT_PV(origin, 2);
    R ivx = LT_PV(inv_voxel, 0), ivy = LT_PV(inv_voxel, 1), ivz = LT_PV(inv_voxel, 2);
    [[maybe_unused]] const R fnx = LT_PV(fdim, 0), fny = LT_PV(fdim, 1), fnz = LT_PV(fdim, 2);      // (mesh kernels in this mode only)
#if LT_INV_MODE == 1
    asm volatile("" : "+v"(gx0), "+v"(gy0), "+v"(gz0), "+v"(ivx), "+v"(ivy), "+v"(ivz));
#endif
#endif

    if constexpr (PHASE == 2) {
        // tail: this wave's 64 pool entries (if there are that many); no queue, no refill
        q_done = true;
        const unsigned have = *P.pool_n < P.pool_cap ? *P.pool_n : P.pool_cap;
        const unsigned e = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 64u + (unsigned)lane;
        if (e < have) {
            const SurvD<R>& S = reinterpret_cast<const SurvD<R>*>(P.pool)[e];
            px = S.p[0]; py = S.p[1]; pz = S.p[2]; ux = S.u[0]; uy = S.u[1]; uz = S.u[2]; w = S.w; sleft = S.sleft;
            cur = S.cur; step = S.step;      // (the id is not needed any more: the trajectory continues from the RNG state)
            __builtin_memcpy(&rng, S.rng, sizeof S.rng);
            alive = true;
#if LT_WALK_BATCH == 1
            if constexpr (!TABLE) {      // a step that was waiting for its surface query when the bulk kernel handed the photon over
                q_pend = S.q_pend != 0u;
                q_u1 = __builtin_bit_cast(typename HeldU<R, TABLE>::type, S.held[0]);
                q_u2 = __builtin_bit_cast(typename HeldU<R, TABLE>::type, S.held[1]);
                q_u3 = __builtin_bit_cast(typename HeldU<R, TABLE>::type, S.held[2]);
            }
#endif
        }
    }
    for (;;) {
        // ---------------- refill dead lanes (ballot + rank) ----------------
        // Refilling costs the whole wave ~140 instructions (seeding + stream warm-up + emission) however few lanes
        // take part, and some lane dies in one wave-step out of five: waiting until kRefillMin lanes are free cuts that
        // overhead fourfold for an average of 1.5 idle lanes.  A photon's fate depends on (seed, id) only, so the
        // results do not change.
        // `alive` lives as a lane mask in a scalar pair, and every ballot of it is a round trip through a VGPR (v_cndmask 0,1 +
        // v_cmp_ne): it is taken ONCE per iteration, here, and the refill test and the loop's exit both read `need`; the two
        // rare blocks that change `alive` after it -- a refill, a hand-over -- ask again.
        unsigned long long need = __ballot(!alive);
        // (the count goes through an empty asm as a 32-bit scalar: left visible, `popcount >= kRefillMin` is widened to a 64-bit
        // ordered compare, which the scalar unit does not have -- v_mov_b64 + v_cmp_*_u64 on the vector pipe)
        unsigned cnt = (unsigned)__popcll(need);
        if constexpr (kSlabForm) asm("" : "+s"(cnt));
        if (need != 0ull && !(q_done && pk_next >= pk_end) && (cnt >= kRefillMin || need == __ballot(true))) {
#if LT_WALK_BATCH && defined(LT_DIAG_MESH)
            dg_refill_it++; dg_refill += cnt;
#endif
            const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32),
                                      __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
            const pk_t avail = pk_end - pk_next;
            unsigned long long nlo = 0, nhi = 0;     // a packet taken from the queue now: ids [nlo, nhi), nnew of them
            pk_t nnew = 0;
            if (cnt > avail && !q_done) {   // the rare dequeue: the only 64-bit arithmetic of the refill
                const int leader = __ffsll((long long)need) - 1;
                unsigned long long base = 0;
                if (lane == leader)
                    base = __hip_atomic_fetch_add(P.head, (unsigned long long)kPacket, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
                base = readlane64(base, leader);
                nlo = base < P.n_photons ? base : P.n_photons;
                nhi = base + kPacket < P.n_photons ? base + kPacket : P.n_photons;
                nnew = (pk_t)(nhi - nlo);
                if (nhi >= P.n_photons) q_done = true;
            }
            bool got = false;
            unsigned long long id = 0;
            if (!alive) {
                if (rank < avail) { id = pk_base + (pk_next + rank); got = true; }
                else if (rank - avail < nnew) { id = nlo + (rank - avail); got = true; }
            }
            if (cnt <= avail) pk_next += cnt;
            else {
                const pk_t used = cnt - avail < nnew ? cnt - avail : nnew;
                if constexpr (kSlabForm) { pk_base = nlo; pk_next = used; pk_end = nnew; }
                else { pk_next = nlo + used; pk_end = nhi; }
            }

            if (got) {
                // ------------- emission: role of sample_light, S/light_samples.py:90-116
                pid = P.photon_offset + id;
                alive = true; w = 1; sleft = 0; step = 0; grp = 0;
                R e_pdf_dir = 1;      // light sub-path capture: density of the emitted direction (pencil beam: 1)
                max_steps = P.max_steps;
                if constexpr (!TABLE) photon_stream(P.seed, pid, &rng);
                if (P.src_type == LT_SRC_COSINE_QUAD) {
                    R u4[4];
                    if constexpr (TABLE) {
                        const double* t = P.table + (id * P.table_steps + grp) * 4;
#pragma unroll
                        for (int k = 0; k < 4; k++) u4[k] = (R)(1.0 - t[k]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; k++) u4[k] = Mx<R>::uniform32(&rng);
                    }
                    grp++;
                    R nrm[3] = {(R)P.src_dir[0], (R)P.src_dir[1], (R)P.src_dir[2]};
                    R o4[4];
                    {
                        const R v2[3] = {s_frame[0], s_frame[1], s_frame[2]}, v3[3] = {s_frame[3], s_frame[4], s_frame[5]};
                        cosine_lobe_frame(nrm, v2, v3, u4[2], u4[3], o4);
                    }
                    e_pdf_dir = Mx<R>::abs(o4[0] * nrm[0] + o4[1] * nrm[1] + o4[2] * nrm[2]) * (R)0.3183098861837907;   // |cos| / pi, S/light_samples.py:83
                    ux = o4[0]; uy = o4[1]; uz = o4[2];
                    px = (R)P.src_pos[0] + u4[0] * (R)P.src_e1[0] + u4[1] * (R)P.src_e2[0] + eps * o4[0];  // :96
                    py = (R)P.src_pos[1] + u4[0] * (R)P.src_e1[1] + u4[1] * (R)P.src_e2[1] + eps * o4[1];
                    pz = (R)P.src_pos[2] + u4[0] * (R)P.src_e1[2] + u4[1] * (R)P.src_e2[2] + eps * o4[2];
                } else {
                    px = (R)P.src_pos[0]; py = (R)P.src_pos[1]; pz = (R)P.src_pos[2];
                    ux = (R)P.src_dir[0]; uy = (R)P.src_dir[1]; uz = (R)P.src_dir[2];
                }
                if constexpr (!MESH) {
                    cur = -1;
                    for (int l = 0; l < P.n_layers; l++)
                        if (pz >= s_zb[l] && pz < s_zb[l + 1]) { cur = l; break; }
                    if (cur < 0) {
                        atomicAdd(&s_cnt[CW_ESC_TOP], (double)w); alive = false;
                    } else if (P.src_type == LT_SRC_PENCIL && pz == s_zb[0] && uz > 0) {
                        R n2 = s_med[s_lm[0]].n, n1 = (R)P.n_above;
                        if (n1 != n2) {  // specular reflection on entering the first layer
                            R d[3] = {ux, uy, uz}, nf[3] = {0, 0, -1}, ct, refr[3];
                            R Rs = boundary(d, nf, n1, n2, &ct, refr);
                            atomicAdd(&s_cnt[CW_SPECULAR], (double)(w * Rs));
                            w -= w * Rs;
                            if (!(w > 0)) alive = false;
                            ux = refr[0]; uy = refr[1]; uz = refr[2];
                        }
                    }
                } else {
                    cur = P.start_medium;
                }
                nv = 0;
                if constexpr (CAPTURE) if (P.vertices) {
                    P.vertex_counts[id] = 0;
                    if (alive) {
                        R pdf_pos = 1;
                        if (P.src_type == LT_SRC_COSINE_QUAD) {     // 1 / area of the quad (S/light_samples.py:100)
                            const R e1[3] = {(R)P.src_e1[0], (R)P.src_e1[1], (R)P.src_e1[2]}, e2[3] = {(R)P.src_e2[0], (R)P.src_e2[1], (R)P.src_e2[2]};
                            R cr[3]; cross3(e1, e2, cr);
                            pdf_pos = (R)1 / Mx<R>::sqrt(dot3(cr, cr));
                        }
                        record_vertex<R>(P, id, nv, px, py, pz, ux, uy, uz, w, LT_VERTEX_LIGHT, cur, 0u, (R)P.src_dir[0], (R)P.src_dir[1],
                                         (R)P.src_dir[2], pdf_pos, e_pdf_dir);
                    }
                }
                if constexpr (TABLE) {
                    unsigned long long cap = P.table_steps > grp ? P.table_steps - grp : 0ull;
                    if (cap < (unsigned long long)max_steps) max_steps = (unsigned)cap;
                }
            }
            need = __ballot(!alive);
        }
        // wave-uniform: queue drained and every lane done (the right-hand side is exec).  In front of the hand-over, which does
        // nothing for a wave without a live lane: kept beyond it, `need` costs the bulk kernel a scalar pair it does not have (the
        // log's pointers were spilled instead, and restored in every append).  The kernels that are not kLean ask `alive` again, below.
        if constexpr (kLean) if (need == __ballot(true)) break;
        // (the empty asm takes the sum here: left alone it sinks to the end of the step, and `need` and a copy of exec live through it)
        if constexpr (kStepsScalar) { steps_w += (unsigned)__popcll(__ballot(true) & ~need); asm volatile("" : "+s"(steps_w)); }      // the live lanes: each steps, or is capped
        if constexpr (PHASE == 1) {
            // bulk: nothing left to refill with and few lanes alive -> hand them over and leave (see "Tail split" above)
            if (q_done && pk_next >= pk_end && !dumped) {
                const unsigned long long am = __ballot(alive);
                const unsigned na = (unsigned)__popcll(am);
                if (na != 0u && na <= P.dump_max) {
                    emit_deposit<TALLY, kRoute>(P, pend_idx, pend_val, lg_cur, lg_end, lg_chunk, s_hist);
                    pend_idx = kNoVoxel;
                    const int leader = __ffsll((long long)am) - 1;
                    unsigned base = 0;
                    if (lane == leader) base = __hip_atomic_fetch_add(P.pool_n, na, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    base = (unsigned)__builtin_amdgcn_readlane((int)base, leader);
                    if (alive) {
                        const unsigned slot = base + __builtin_amdgcn_mbcnt_hi((unsigned)(am >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)am, 0u));
                        if (slot < P.pool_cap) {      // (the pool holds kDumpPoolLanes >= dump_max entries per launched wave: it cannot overflow)
                            SurvD<R>& S = reinterpret_cast<SurvD<R>*>(P.pool)[slot];
                            S.p[0] = px; S.p[1] = py; S.p[2] = pz; S.u[0] = ux; S.u[1] = uy; S.u[2] = uz; S.w = w; S.sleft = sleft;
                            S.pid = 0ull; S.cur = cur; S.step = step;
                            __builtin_memcpy(S.rng, &rng, sizeof S.rng);
#if LT_WALK_BATCH == 1
                            if constexpr (!TABLE) {
                                S.q_pend = q_pend ? 1u : 0u;
                                S.held[0] = __builtin_bit_cast(uint32_t, q_u1); S.held[1] = __builtin_bit_cast(uint32_t, q_u2);
                                S.held[2] = __builtin_bit_cast(uint32_t, q_u3);
                                q_pend = false;
                            }
#else
                            S.q_pend = 0u;
#endif
                            alive = false;
                        }
                    }
                    dumped = true;
                    if constexpr (kStepsScalar) {      // (the lanes handed over take no step here: off the count they were just put on)
                        const unsigned long long left = __ballot(alive);
                        steps_w -= na - (unsigned)__popcll(left);
                        if (left == 0ull) break;
                    } else if constexpr (kLean) if (!__any(alive)) break;
                }
            }
        }
        if constexpr (!kLean) if (!__any(alive)) break;  // wave-uniform: queue drained and every lane done

#if LT_WALK_BATCH == 2
        // ---------------- one photon-step ----------------
        // (A) prepare, for the lanes that are not in a query: uniforms, free path, clearance test.  A hop that may reach a
        // surface becomes a query: the prepared step is held (as in walk_kernel_q) and the lane's ray enters the march.
        // (B) march_round: every query in flight visits ONE cell and queues its candidates; when enough have gathered (or
        // nothing else is left to do) the whole wave tests them (march_drain).  (C) a query whose march has ended and whose
        // candidates have all been tested completes its step with the lanes whose hop needed no query.  Nobody waits for a
        // service: a wave iteration always advances every lane, a step or a cell.  A photon's own sequence of operations is
        // what it is in walk_kernel_q -- only the interleaving with its neighbours changes -- so results are bit for bit.
        unsigned f_idx = kNoVoxel;  // deposit record leaving the run-length accumulator this step
        TV f_val = 0;
        bool go = false;
        R u1 = 0, s = 0, tb = inf;
        typename HeldU<R, TABLE>::type x2 = 0, x3 = 0;      // the step's fourth uniform as drawn (f64 XORWOW: raw; converted where a decision needs it)
        int hit_tri = -1;
#if defined(LT_DIAG_MESH)
        const long long dgm_t0 = clock64();
        dg_iter++; dg_alive += __popcll(__ballot(alive)); dg_prep += __popcll(__ballot(alive && !q_pend));
#endif
        if (alive && !q_pend) {
            if (step >= max_steps) {
                atomicAdd(&s_cnt[CW_CAPPED], (double)w); alive = false;
            } else {
                step++;
                acc_steps++;
                const float clr = march_clearance<R>(P.mg, px, py, pz);   // requested early: ~150 instructions hide its latency
                const typename HeldU<R, TABLE>::type x0 = HeldU<R, TABLE>::draw(&rng);      // (free path: taken from the raw draw)
                u1 = Mx<R>::uniform32(&rng);
                x2 = HeldU<R, TABLE>::draw(&rng);
                x3 = HeldU<R, TABLE>::draw(&rng);
                grp++;
                const MedD<R>* Mq = LT_MED(cur);
                if (sleft == 0) sleft = HeldU<R, TABLE>::neg_log(x0, s_math);
                s = (Mq->mu_t > 0) ? sleft * Mq->inv_mu_t : inf;
                if (!(s < (R)clr)) {
                    q_pend = true;
                    mw->held[0][lane] = s; mw->held[1][lane] = u1; mw->held[2][lane] = HeldU<R, TABLE>::as_real(x2); mw->held[3][lane] = HeldU<R, TABLE>::as_real(x3);
                    q_tc = clr > 0.0f ? (R)clr : (R)0;      // the march starts where the clearance of this cell ends
                    q_march = march_enter<R>(P.mg, mw, px, py, pz, ux, uy, uz, s);
                    q_bvh = !q_march; q_dirty = false;
                } else go = true;
            }
        }
        {
            bool full = false;
#if defined(LT_DIAG_MESH)
            const long long dgm_t1 = clock64();
            dgm_clk[0] += dgm_t1 - dgm_t0;
            { const unsigned long long m_ = __ballot(q_march); if (m_) { dg_trav_it++; dg_trav += __popcll(m_); } }
#endif
            if (__any(q_march)) {
                bool heavy = false;
                full = march_round<R>(P.mg, mw, q_march, heavy, q_dirty, q_tc, mq_n);
                q_bvh = q_bvh || heavy;
            }
#if defined(LT_DIAG_MESH)
            const long long dgm_t2 = clock64();
            dgm_clk[1] += dgm_t2 - dgm_t1;
#endif
            // drain when a full round of candidates waits, the queue is full, enough queries wait for nothing else, or no
            // lane of the wave can do anything else
            const unsigned long long wm = __ballot(q_pend && !q_march && q_dirty);
            if (mq_n > 0 && (full || mq_n >= 64u || (unsigned)__popcll(wm) >= drain_min || !__any(go || q_march))) {
#if defined(LT_DIAG_MESH)
                dg_bvh_it++; dg_bvh += mq_n;
#endif
                march_drain<R>(s_tris, P.mg, mw, mq_n);
                q_dirty = false;
            }
#if defined(LT_DIAG_MESH)
            const long long dgm_t3 = clock64();
            dgm_clk[2] += dgm_t3 - dgm_t2;
#endif
            if (q_pend && !q_march && !q_dirty) {
                s = mw->held[0][lane]; u1 = mw->held[1][lane]; x2 = HeldU<R, TABLE>::from_real(mw->held[2][lane]); x3 = HeldU<R, TABLE>::from_real(mw->held[3][lane]);
                R th;
                march_result<R>(s_tris, s_nodes, P.n_nodes, s_links, mw, q_bvh, px, py, pz, ux, uy, uz, s, hit_tri, th);
                if (hit_tri >= 0) tb = th;
                q_pend = false; q_bvh = false; go = true;
            }
#if defined(LT_DIAG_MESH)
            dgm_clk[3] += clock64() - dgm_t3;
#endif
        }
#if defined(LT_DIAG_MESH)
        const long long dg_t1 = clock64();
        {
            const unsigned long long gm = __ballot(go), bm = __ballot(go && hit_tri >= 0);
            dg_go += __popcll(gm);
            if (bm) { dg_bnd_it++; dg_bnd += __popcll(bm); }
            if (gm & ~bm) { dg_int_it++; dg_int += __popcll(gm & ~bm); }
        }
#endif
        if (go) {
            {
                const MedD<R>* Mp = LT_MED(cur);
                const R mu_t = Mp->mu_t;
#elif LT_WALK_BATCH
        // ---------------- one photon-step ----------------
        // Three stages.  (A) prepare: uniforms, free path, and for a mesh the clearance test.  (B) mesh only: the
        // surface query -- the cell's listed nearest triangles when the hop cannot reach any other (98 % of the
        // queries on the Cornell cavity), the BVH otherwise (nearest_listed).  Whenever ANY lane of a wave needs it the
        // whole wave pays for it, at the occupancy of the lanes that asked (PMC: 24 % lane utilisation on the Cornell
        // cavity before this), so lanes that need a query hold their prepared step and wait until query_min of them have
        // gathered -- or until no lane of the wave can advance without one.  (C) complete: boundary event or
        // interaction.  A photon's own sequence of operations is unchanged, only its interleaving with its neighbours',
        // so the results are too.
        unsigned f_idx = kNoVoxel;  // deposit record leaving the run-length accumulator this step
        TV f_val = 0;
        bool go = false;
        R u1 = 0, s = 0, tb = inf;
        typename HeldU<R, TABLE>::type x2 = 0, x3 = 0;      // the step's fourth uniform as drawn (f64 XORWOW: raw; converted where a decision needs it)
        int hit_tri = -1;
#if defined(LT_DIAG_MESH)
        dg_iter++; dg_alive += __popcll(__ballot(alive)); dg_prep += __popcll(__ballot(alive && !(MESH && q_pend)));
#endif
        if (alive && !(MESH && q_pend)) {
            if (step >= max_steps) {
                atomicAdd(&s_cnt[CW_CAPPED], (double)w); alive = false;
            } else {
                step++;
                acc_steps++;
                // mesh walks: the clearance of the current cell is a dependent global load; requested here, before the
                // ~150 instructions of RNG and logarithm, its latency is hidden by the time the hop length is known
                float clr = -1.0f;   // no grid / outside it: always query
                unsigned rec_y = 0u, rec_z = 0xffffffffu;      // (no record: c2 = 0, no triangles listed)
                if constexpr (GEOM == 2) {
                    if (P.mg.cell) clr = march_clearance<R>(P.mg, px, py, pz);
                } else if constexpr (MESH) {
                    if (P.clear) {
                        const R cx = (px - LT_PV(corg, 0)) * LT_PV(cinv, 0), cy = (py - LT_PV(corg, 1)) * LT_PV(cinv, 1),
                                cz = (pz - LT_PV(corg, 2)) * LT_PV(cinv, 2);
                        if (cx >= 0 && cx < LT_PV(cdim, 0) && cy >= 0 && cy < LT_PV(cdim, 1) && cz >= 0 && cz < LT_PV(cdim, 2)) {
                            const uint4 rec = P.clear[((size_t)(int)cz * P.cny + (int)cy) * P.cnx + (int)cx];
                            clr = __uint_as_float(rec.x); rec_y = rec.y; rec_z = rec.z;
                        }
                    }
                }
                typename HeldU<R, TABLE>::type x0, h1, h2, h3;      // the step's uniforms as drawn; h1..h3 are what a waiting step holds
                if constexpr (TABLE) {  // table RNG: S/scene.py:68-69, S/path_tracing_fix1.py:28-29
                    const double* t = P.table + ((pid - P.photon_offset) * P.table_steps + grp) * 4;
                    x0 = (R)(1.0 - t[0]); h1 = (R)(1.0 - t[1]); h2 = (R)(1.0 - t[2]); h3 = (R)(1.0 - t[3]);
                } else if constexpr (sizeof(R) == 8) {   // four uniforms of 32-bit resolution: 4 XORWOW draws per step (2^-32 is e^-22 on the free-path scale)
                    x0 = rocrand(&rng); h1 = rocrand(&rng); h2 = rocrand(&rng); h3 = rocrand(&rng);
                } else {
                    x0 = Mx<R>::uniform32(&rng); h1 = Mx<R>::uniform32(&rng); h2 = Mx<R>::uniform32(&rng); h3 = HeldU<R, TABLE>::draw(&rng);
                }
                u1 = HeldU<R, TABLE>::get(h1); x2 = h2; x3 = h3;
                grp++;
                const MedD<R>* Mq = LT_MED(MESH ? cur : s_lm[cur]);
                if (sleft == 0) sleft = HeldU<R, TABLE>::neg_log(x0, s_math);
                s = (Mq->mu_t > 0) ? sleft * Mq->inv_mu_t : inf;

                // ---- hop: distance to the next boundary ----
                if constexpr (!MESH) {
                    if (uz != 0) {
                        const R dz = (uz > 0 ? s_zb[cur + 1] : s_zb[cur]) - pz;   // sign of uz, or 0
                        // A hop that ends well inside the layer needs no quotient: |dz| > s |uz| (1 + d) with
                        // d >= 8 ulp implies fl(dz / uz) > s, so `tb <= s` below is false either way and tb is
                        // not read.  Only lanes within a step of an interface pay for the IEEE division.
                        const R guard = sizeof(R) == 8 ? (R)(1.0 + 1e-12) : (R)(1.0 + 1e-5);
                        const bool near = !(Mx<R>::abs(dz) > s * Mx<R>::abs(uz) * guard);
                        if (__any(near)) {   // wave-uniform skip; the empty asm keeps the quotient from being hoisted
                            R den = uz;      // back out and turned into a select
                            asm volatile("" : "+v"(den));
                            if (near) tb = dz / den;
                        }
                    }
                    go = true;
                } else {
                    // clearance grid: every triangle is farther than `c` from every point of this cell, so a hop of
                    // length s < c ends before any surface and the traversal is skipped (same result, no query)
                    if (!(s < (R)clr)) {
                        // ... and a hop shorter than the cell's c2 can only hit the two triangles the record lists: if it cannot
                        // even reach their planes (plane_within_reach: a rejection in front of tri_hit that never rejects a hop
                        // tri_hit would accept -- in f32 by the slack the host derived from the mesh) there is no query
                        bool need = true;
                        if constexpr (GEOM == 1) {
                            const float c2 = (float)__builtin_bit_cast(_Float16, (unsigned short)(rec_y & 0xffffu));
                            if (s < (R)c2) {
                                const unsigned i0 = rec_z & 0xffffu, i1 = rec_z >> 16;
                                R kslack = 0;
                                if constexpr (sizeof(R) == 4) kslack = P.reach_slack;
                                need = (i0 != 0xffffu && plane_within_reach(&s_tris[i0], px, py, pz, ux, uy, uz, s, kslack)) ||
                                       (i1 != 0xffffu && plane_within_reach(&s_tris[i1], px, py, pz, ux, uy, uz, s, kslack));
                            }
                        }
                        if (need) { q_pend = true; q_u1 = h1; q_u2 = h2; q_u3 = h3; }
                        else go = true;
                    } else go = true;
                }
            }
        }
        if constexpr (MESH) {
            const unsigned long long wq = __ballot(q_pend);
#if defined(LT_DIAG_MESH)
            if (wq != 0ull && ((unsigned)__popcll(wq) >= query_min || q_age + 1 > kQueryMaxAge || !__any(go))) { dg_trav_it++; dg_trav += __popcll(wq); }
            else dg_wait += __popcll(wq);
#endif
            // ... or until the oldest of them has waited kQueryMaxAge iterations: where queries are rare a wave would
            // otherwise idle its waiting lanes until enough of them have trickled in
            if (wq != 0ull) q_age++;
            if (wq != 0ull && ((unsigned)__popcll(wq) >= query_min || q_age > kQueryMaxAge || !__any(go))) {
                q_age = 0;
#if defined(LT_DIAG_MESH)
                const long long dg_t0 = clock64();
#endif
                if (q_pend) {
                    {
                        const MedD<R>* Mq = LT_MED(MESH ? cur : s_lm[cur]);
                        s = (Mq->mu_t > 0) ? sleft * Mq->inv_mu_t : inf;
                    }
                    u1 = HeldU<R, TABLE>::get(q_u1); x2 = q_u2; x3 = q_u3;
                    R o[3] = {px, py, pz}, d[3] = {ux, uy, uz}, th;
                    if constexpr (GEOM == 2) {
                        nearest_bvh_walk(s_tris, s_nodes, P.n_nodes, s_links, o, d, s, hit_tri, th);
                    } else {
                    // the cell's record again (the position has not moved while the step waited): which triangles
                    // are within reach of this hop
                    uint4 rec = make_uint4(0u, 0u, 0xffffffffu, 0xffffffffu);
                    if (P.clear) {
                        const R cx = (px - LT_PV(corg, 0)) * LT_PV(cinv, 0), cy = (py - LT_PV(corg, 1)) * LT_PV(cinv, 1),
                                cz = (pz - LT_PV(corg, 2)) * LT_PV(cinv, 2);
                        if (cx >= 0 && cx < LT_PV(cdim, 0) && cy >= 0 && cy < LT_PV(cdim, 1) && cz >= 0 && cz < LT_PV(cdim, 2))
                            rec = P.clear[((size_t)(int)cz * P.cny + (int)cy) * P.cnx + (int)cx];
                    }
#if defined(LT_DIAG_MESH)
                    {
                        const float c2_ = (float)__builtin_bit_cast(_Float16, (unsigned short)(rec.y & 0xffffu));
                        const float c4_ = (float)__builtin_bit_cast(_Float16, (unsigned short)(rec.y >> 16));
                        const unsigned long long fb = __ballot(!(s < (R)c4_)), f4 = __ballot(!(s < (R)c2_) && s < (R)c4_);
                        if (fb) { dg_bvh_it++; dg_bvh += __popcll(fb); }
                        if (f4) { dg_l4_it++; dg_l4 += __popcll(f4); }
                    }
#endif
                    nearest_listed(s_tris, s_nodes, P.n_nodes, s_links, rec, o, d, s, hit_tri, th);
                    }
                    if (hit_tri >= 0) tb = th;
                    q_pend = false; go = true;
                }
#if defined(LT_DIAG_MESH)
                dg_clk_srv += clock64() - dg_t0;
#endif
            }
        }
#if defined(LT_DIAG_MESH)
        {
            const unsigned long long gm = __ballot(go), bm = __ballot(go && hit_tri >= 0);
            dg_go += __popcll(gm);
            if (bm) { dg_bnd_it++; dg_bnd += __popcll(bm); }
            if (gm & ~bm) { dg_int_it++; dg_int += __popcll(gm & ~bm); }
        }
#endif
#if defined(LT_DIAG_MESH)
        const long long dg_t1 = clock64();
#endif
        if (go) {
            {
                const MedD<R>* Mp = LT_MED(MESH ? cur : s_lm[cur]);
                const R mu_t = Mp->mu_t;
#else
        // ---------------- one photon-step ----------------
        unsigned f_idx = kNoVoxel;  // deposit record leaving the run-length accumulator this step
        // Its value is read only where f_idx names a voxel.  A default would be written on every path of the step that does not
        // set it (three per wave-step in the ISA), so it is defined without code, by an empty asm with an output only.  (Not the
        // vertex capture, nor the mesh kernels: there the definition's longer life costs a register they do not have.)
        TV f_val;
        if constexpr (kLean) asm volatile("" : "=v"(f_val)); else f_val = 0;
        if (alive) {
            if (step >= max_steps) {
                atomicAdd(&s_cnt[CW_CAPPED], (double)w); alive = false;
                if constexpr (kStepsScalar) atomicAdd(reinterpret_cast<unsigned long long*>(lds_raw + LdsLayout<R>::kSlabCap), 1ull);
            } else {
                step++;
                if constexpr (!kStepsScalar) acc_steps++;
                // mesh walks: the clearance of the current cell is a dependent global load; requested here, before the
                // ~150 instructions of RNG and logarithm, its latency is hidden by the time the hop length is known
                float clr = -1.0f;   // no grid / outside it: always query
                if constexpr (GEOM == 2) {
                    if (P.mg.cell) clr = march_clearance<R>(P.mg, px, py, pz);
                } else if constexpr (MESH) {
                    if (P.clear) {
                        const R cx = (px - LT_PV(corg, 0)) * LT_PV(cinv, 0), cy = (py - LT_PV(corg, 1)) * LT_PV(cinv, 1),
                                cz = (pz - LT_PV(corg, 2)) * LT_PV(cinv, 2);
                        if (cx >= 0 && cx < LT_PV(cdim, 0) && cy >= 0 && cy < LT_PV(cdim, 1) && cz >= 0 && cz < LT_PV(cdim, 2))
                            clr = __uint_as_float(P.clear[((size_t)(int)cz * P.cny + (int)cy) * P.cnx + (int)cx].x);
                    }
                }
                R u1;
                typename HeldU<R, TABLE>::type x0, x2, x3;      // the step's fourth uniform as drawn (f64 XORWOW: raw; converted where a decision needs it)
                if constexpr (TABLE) {  // table RNG: S/scene.py:68-69, S/path_tracing_fix1.py:28-29
                    const double* t = P.table + ((pid - P.photon_offset) * P.table_steps + grp) * 4;
                    x0 = (R)(1.0 - t[0]); u1 = (R)(1.0 - t[1]); x2 = (R)(1.0 - t[2]); x3 = (R)(1.0 - t[3]);
                } else {   // four uniforms of 32-bit resolution: 4 XORWOW draws per step (2^-32 is e^-22 on the free-path scale)
                    x0 = HeldU<R, TABLE>::draw(&rng);      // free path and azimuth are taken from the RAW draws (neg_log_raw, sincos_turn_raw)
                    u1 = Mx<R>::uniform32(&rng);
                    x2 = HeldU<R, TABLE>::draw(&rng);
                    x3 = HeldU<R, TABLE>::draw(&rng);      // the fourth stays a raw draw until a boundary decision or the roulette asks for it
                }
                grp++;
                // Slab walks: everything the step reads about its layer is ONE record (LayD) whose address follows from `cur`
                // alone, and the cells of the two math tables follow from the draws alone, so all of these reads are issued HERE, at
                // the top of the step, and each is waited for where its value is first used.  The empty asm is a compiler barrier
                // without operands: no read moves below it (left alone, each read sinks into the block that uses it and is waited for
                // on the next line), and since it names no register nothing is waited for at it.  Two builds read the interaction's
                // fields and the table cells where they use them, for want of registers to hold them in: the tail kernel (PHASE 2),
                // which runs beside the log reduction in the registers that leaves, and the vertex capture.
                // LT_LAY_LATE / LT_TAB_LATE: measurement builds without the early record / table reads.
                static_assert(!MESH, "walk_kernel is the slab walk");
                constexpr bool kLayEarly = PHASE != 2 && !CAPTURE && !LT_LAY_LATE;
                constexpr bool kTabEarly = !TABLE && sizeof(R) == 8 && PHASE != 2 && !CAPTURE && !LT_TAB_LATE;
                [[maybe_unused]] const MedD<R>* Mp = s_med;      // (the mesh branches of the shared text below; never built into this kernel)
                const LayD<R>* Yp = LT_LAY(cur);
                const R mu_t = Yp->mu_t, inv_mu_t = Yp->inv_mu_t, z_lo = Yp->z_lo, z_hi = Yp->z_hi;
                [[maybe_unused]] R absorb = 0, dep = 0, hg_2g = 0, hg_1mg = 0, hg_1mg2 = 0, hg_1pg2 = 0, hg_i2g = 0;
                [[maybe_unused]] double2 Tln, Tsc;
                if constexpr (kTabEarly) { Tln = neg_log_cell(x0, s_math); Tsc = sincos_turn_cell(x2, s_math); }
                if constexpr (kLayEarly) {
                    absorb = Yp->absorb; dep = Yp->dep;
                    hg_2g = Yp->two_g; hg_1mg = Yp->one_m_g; hg_1mg2 = Yp->one_m_g2; hg_1pg2 = Yp->one_p_g2; hg_i2g = Yp->inv_2g;
                }
                if constexpr (kLayEarly || kTabEarly) asm volatile("" ::: "memory");
                if (sleft == 0) {
                    if constexpr (kTabEarly) sleft = neg_log_raw(x0, Tln); else sleft = HeldU<R, TABLE>::neg_log(x0, s_math);
                }
                const R s = (mu_t > 0) ? sleft * inv_mu_t : inf;

                // ---- hop: distance to the next boundary ----
                // Whether the hop ends on an interface is carried as a mask: `near` lanes whose quotient is <= s (a NaN quotient, 0 / 0,
                // is not), empty where no lane of the wave is near.  tb is read by those lanes alone, so it has no default: an
                // infinity written in front of the hop and again in the no-lane-near arm was four moves and an all-lane compare per
                // step.  (The one lane that is not near and yet passed `inf <= inf` -- uz == 0 in a medium without interaction, s == inf:
                // with uz != 0 an infinite s makes every lane near -- is given its infinity and its bit in the arm of `uz != 0`.)
                R tb; int hit_tri = -1;
                bool hop_ends_at_plane = false;
                if constexpr (kDiet && kLean) asm volatile("" : "=v"(tb)); else tb = inf;
                if constexpr (!MESH) {
                    if (uz != 0) {
                        const R dz = (uz > 0 ? z_hi : z_lo) - pz;   // the layer's own bounds, from its record: sign of uz, or 0
                        // A hop that ends well inside the layer needs no quotient: |dz| > s |uz| (1 + d) with
                        // d >= 8 ulp implies fl(dz / uz) > s, so `tb <= s` below is false either way and tb is
                        // not read.  Only lanes within a step of an interface pay for the IEEE division.
                        const R guard = sizeof(R) == 8 ? (R)(1.0 + 1e-12) : (R)(1.0 + 1e-5);
                        const bool near = !(Mx<R>::abs(dz) > s * Mx<R>::abs(uz) * guard);
                        if (__any(near)) {   // wave-uniform skip; the empty asm keeps the quotient from being hoisted
                            R den = uz;      // back out and turned into a select
                            asm volatile("" : "+v"(den));
                            if (near) { tb = dz / den; if constexpr (kDiet) hop_ends_at_plane = tb <= s; }
                        }
                    } else if constexpr (kDiet) {
                        if (s == inf) { tb = inf; hop_ends_at_plane = true; }      // uz == 0 and no interaction: `inf <= inf`, as ever
                    }
                } else {
                    // clearance grid: every triangle is farther than `c` from every point of this cell, so a hop of
                    // length s < c ends before any surface and the traversal is skipped (same result, no query)
                    const bool query = !(s < (R)clr);
                    if (query) {
                        R o[3] = {px, py, pz}, d[3] = {ux, uy, uz}, th;
                        nearest_bvh_walk(s_tris, s_nodes, P.n_nodes, s_links, o, d, s, hit_tri, th);
                        if (hit_tri >= 0) tb = th;
                    }
                }
                const bool at_boundary = kDiet ? hop_ends_at_plane : (tb <= s);
#endif
#if LT_WALK_BATCH
                const bool at_boundary = MESH ? (hit_tri >= 0) : (tb <= s);
#endif
                if (!at_boundary && !(s < inf)) {
                    atomicAdd(&s_cnt[MESH ? CW_ESC_MESH : CW_CAPPED], (double)w); alive = false;
                } else if (at_boundary) {
                    px += ux * tb; py += uy * tb; pz += uz * tb;
                    sleft -= tb * mu_t;
                    if (!(sleft > 0)) sleft = 0;
                    if constexpr (!MESH) {
                        // plane interface k (IfD: both indices and their quotients from the host): see boundary_planar
                        const bool down = uz > 0;
                        const int k = down ? cur + 1 : cur, next = down ? cur + 1 : cur - 1;
                        pz = s_zb[k];
                        const IfD<R> F = s_if[k];
                        const R Nr = down ? F.nr_down : F.nr_up;
                        R ct;
                        const R Rf = boundary_planar(uz, down ? F.n_up : F.n_dn, down ? F.n_dn : F.n_up, Nr, &ct);
                        const bool refl = HeldU<R, TABLE>::get(x3) <= Rf;
                        const bool gone = !refl && (next < 0 || next >= P.n_layers);
                        if constexpr (CAPTURE) if (P.vertices)     // a delta event: pdf_dir = probability of the branch taken (0: the photon leaves the scene)
                            record_vertex<R>(P, pid - P.photon_offset, nv, px, py, pz, ux, uy, uz, w,
                                             refl ? LT_VERTEX_REFLECTIVE : LT_VERTEX_TRANSMISSIVE, cur, step, (R)0, (R)0, down ? (R)-1 : (R)1, (R)0,
                                             gone ? (R)0 : (refl ? Rf : (R)1 - Rf));
                        if (refl) uz = -uz;                        // S/brdf.py:8-9 at a plane
                        else if (gone) { atomicAdd(&s_cnt[next < 0 ? CW_ESC_TOP : CW_ESC_BOT], (double)w); alive = false; }
                        else { ux *= Nr; uy *= Nr; uz = down ? ct : -ct; cur = next; }      // S/path_tracing_fix1.py:107-114 at a plane
                    } else {
                    R nf[3], n1 = Mp->n, n2; int next;
                    {
                        const TriD<R>* T = &s_tris[hit_tri];
                        R tn[3] = {T->n[0], T->n[1], T->n[2]};
                        R d[3] = {ux, uy, uz};
                        R dn = dot3(d, tn);
                        R sg = dn > 0 ? (R)-1 : (R)1;  // S/path_tracing_fix1.py:48-51
                        nf[0] = sg * tn[0]; nf[1] = sg * tn[1]; nf[2] = sg * tn[2];
                        next = dn > 0 ? T->med_front : T->med_back;
                        n2 = next >= 0 ? s_med[next].n : n1;  // exterior: index matched
                    }
                    R d[3] = {ux, uy, uz}, ct, refr[3];
                    R Rf = boundary(d, nf, n1, n2, &ct, refr);
                    if constexpr (CAPTURE) if (P.vertices) {    // a delta event: pdf_dir = probability of the branch taken (0: the photon leaves the scene)
                        const bool refl = HeldU<R, TABLE>::get(x3) <= Rf;
                        const bool leaves = !refl && next < 0;
                        record_vertex<R>(P, pid - P.photon_offset, nv, px, py, pz, ux, uy, uz, w,
                                         refl ? LT_VERTEX_REFLECTIVE : LT_VERTEX_TRANSMISSIVE, cur, step, nf[0], nf[1], nf[2], (R)0,
                                         leaves ? (R)0 : (refl ? Rf : (R)1 - Rf));
                    }
                    if (HeldU<R, TABLE>::get(x3) <= Rf) {  // reflect: S/brdf.py:8-9
                        R ro[3]; reflect_walk(d, nf, ro);
                        ux = ro[0]; uy = ro[1]; uz = ro[2];
                        px += eps * nf[0]; py += eps * nf[1]; pz += eps * nf[2];  // :118
                    } else if (next < 0) {
                        atomicAdd(&s_cnt[CW_ESC_MESH], (double)w); alive = false;
                    } else {
                        ux = refr[0]; uy = refr[1]; uz = refr[2];
                        px -= eps * nf[0]; py -= eps * nf[1]; pz -= eps * nf[2];  // :112
                        cur = next;
                    }
                    }
                } else {
                    // ---- interaction site: move, drop, spin, roulette ----
                    px += ux * s; py += uy * s; pz += uz * s;
                    sleft = 0;
                    const R dw = w * LT_STEP_ABSORB;
                    if constexpr (CAPTURE) if (P.vertices) {    // pdf_dir = the reference's henyey_greenstein at the deflection the spin below samples (its sign
                                         // convention: -cos); recomputed here so that the capture costs the plain walk no register
                        const R ct_c = LT_STEP_HG(u1);
                        record_vertex<R>(P, pid - P.photon_offset, nv, px, py, pz, ux, uy, uz, w, LT_VERTEX_VOLUME, cur, step, (R)0, (R)0, (R)0,
                                         (R)0, (w - dw > 0) ? hg_pdf(-ct_c, LT_STEP_G) : (R)0);
                    }
                    const R fx = (px - gx0) * ivx, fy = (py - gy0) * ivy, fz = (pz - gz0) * ivz;
                    // branch-free: nearly every deposit is inside the grid, so the index is computed for all lanes
                    // and the run-length accumulator is updated with selects
                    // inside the grid: no coordinate negative (the sign bits: the conversion below truncates towards zero, so
                    // (-1, 0) would land in voxel 0) and every truncated coordinate below its dimension -- three integer
                    // compares instead of six in walk precision.  (The conversion saturates; a -0.0 coordinate counts as outside.)
                    const unsigned vx = (unsigned)(int)fx, vy = (unsigned)(int)fy, vz = (unsigned)(int)fz;
                    // (slab kernels; the mesh kernels' scalar file has no room for the three dimensions: they compare in walk
                    //  precision against the copies they keep in LDS)
                    bool inside;
                    if constexpr (kDimLds) {
                        // the three dimensions by one 16-byte LDS read at a constant address (kSlabDim): no VALU instruction and no
                        // scalar register held over the loop
                        const uint4 gd = *reinterpret_cast<const uint4*>(lds_raw + LdsLayout<R>::kSlabDim);
                        // (the sign words pass through an empty asm: left visible, the compiler widens the f64 test to both words of
                        //  each coordinate -- two v_or3_b32 and a 64-bit compare for one v_or3_b32 and a 32-bit one)
                        unsigned sg = Mx<R>::sign_word(fx) | Mx<R>::sign_word(fy) | Mx<R>::sign_word(fz);
                        if constexpr (LT_DIET_SIGN32 != 0) asm("" : "+v"(sg));
                        inside = (int)sg >= 0 && vx < gd.x && vy < gd.y && vz < gd.z;
                    } else if constexpr (!MESH) inside = (int)(Mx<R>::sign_word(fx) | Mx<R>::sign_word(fy) | Mx<R>::sign_word(fz)) >= 0 &&
                                                  vx < (unsigned)P.nx && vy < (unsigned)P.ny && vz < (unsigned)P.nz;
                    else inside = fx >= 0 && fx < fnx && fy >= 0 && fy < fny && fz >= 0 && fz < fnz;
                    // the tile of the voxel (log mode).  <= 65536 tiles, so on a lane inside the grid every factor and sum is below
                    // 2^24 (a lane outside it gets a meaningless index, which is not used).  Slab walks: two v_mad_u32_u24 (mad_u24).
                    // Mesh walks: __umul24 compiles to two v_mad_u64_u32 here -- the compiler keeps only the low 18 bits of the
                    // product and with that forgets the factors' width; the probe prices the two forms alike.
                    // The index: tiled on the log route (see kTileBX), linear on the atomic one; a slab build holds its route's alone
                    // (the log's linear index exists only where an exhausted log spills, log_spill).
                    unsigned idx;
                    if constexpr (kRoute == kRouteAtomic) idx = (vz * (unsigned)P.ny + vy) * (unsigned)P.nx + vx;
                    else {
                        unsigned tile;
                        if constexpr (kSlabForm) tile = mad_u24(mad_u24(vz >> kTileBZ, P.log_nty, vy >> kTileBY), P.log_ntx, vx >> kTileBX);
                        else tile = __umul24(__umul24(vz >> kTileBZ, P.log_nty) + (vy >> kTileBY), P.log_ntx) + (vx >> kTileBX);
                        idx = kRoute == kRouteLog || P.log_idx
                            ? ((tile << kTileShift) | ((vz & 15u) << 10) | ((vy & 31u) << 5) | (vx & 31u))
                            : (vz * (unsigned)P.ny + vy) * (unsigned)P.nx + vx;
                    }
                    const TV q = tally_quantum<TALLY, R>(w * LT_STEP_DEP);     // the tally quantity: absorbed weight, or w / mu_t (fluence)
                    const bool same = inside && idx == pend_idx;
                    const bool flush = inside && !same;
                    f_idx = flush ? pend_idx : kNoVoxel; f_val = pend_val;
                    if constexpr (kDiet) {
                        // One sum for both cases: onto the run (same voxel) or onto zero (a new run), kept where the lane is inside.
                        // Where the tally has the walk's type the product was contracted into the sum, pend_val + w dep in one FMA,
                        // and the new run's value was a second product; now the one FMA serves both: fma(w, dep, +0) rounds as
                        // w dep does, and w > 0, dep >= 0, so no -0 arises.  The other tallies add the quantum: 0 + q is q.
                        // The plain walks: the lanes inside take the sum, the new index and the absorbed weight under their mask and
                        // the others the lost weight under its complement -- x + 0.0 is x, and the sums start at +0.0 -- instead of
                        // eight selects between them.
                        if constexpr (kMaskSum) {
                            if (inside) {
                                const TV base = same ? pend_val : (TV)0;
                                if constexpr (std::is_same<TV, R>::value) pend_val = Mx<R>::fma(w, LT_STEP_DEP, base); else pend_val = base + q;
                                pend_idx = idx;      // (same: the index it holds)
                                acc_abs += (double)dw;
                            } else acc_lost += (double)dw;
                        } else {
                            const TV base = flush ? (TV)0 : pend_val;
                            TV t;
                            if constexpr (std::is_same<TV, R>::value) t = Mx<R>::fma(w, LT_STEP_DEP, base); else t = base + q;
                            pend_val = inside ? t : pend_val;
                        }
                    } else
                    pend_val = same ? pend_val + q : (flush ? q : pend_val);
                    if constexpr (!kMaskSum) {
                        pend_idx = flush ? idx : pend_idx;
                        acc_abs += inside ? (double)dw : 0.0;
                        acc_lost += inside ? 0.0 : (double)dw;
                    }
                    w = sub_rounded(w, dw);
                    if (!(w > 0)) alive = false;
                    else {
                        R u[3] = {ux, uy, uz};
#if LT_WALK_BATCH == 0
                        if constexpr (kTabEarly) {
                            R sp, cp; sincos_turn_raw(x2, Tsc, &sp, &cp);
                            spin_turn<R, true>(u, LT_STEP_HG(u1), sp, cp);       // (hg_sample_walk returns |cos| <= 1)
                        } else
#endif
                        spin<R, TABLE, true>(u, LT_STEP_HG(u1), x2, s_math);
                        ux = u[0]; uy = u[1]; uz = u[2];
                        if (w < (R)1e-4) {  // weight roulette; shape of S/path_tracing_fix1.py:126-132
                            if (HeldU<R, TABLE>::get(x3) <= (R)0.1) { atomicAdd(&s_cnt[CW_ROULETTE], -9.0 * (double)w); w *= (R)10; }
                            else { atomicAdd(&s_cnt[CW_ROULETTE], (double)w); alive = false; }
                        }
                    }
                }
            }
        }
#if LT_WALK_BATCH && defined(LT_DIAG_MESH)
        dg_clk_bnd += clock64() - dg_t1;
#endif
        // wave-uniform point: send this step's records to the grid (atomics) or to the deposit log
        emit_deposit<TALLY, kRoute>(P, f_idx, f_val, lg_cur, lg_end, lg_chunk, s_hist);
    }
    emit_deposit<TALLY, kRoute>(P, pend_idx, pend_val, lg_cur, lg_end, lg_chunk, s_hist);
    if (LT_HAS_LOG && lg_chunk < kLogExhausted && (threadIdx.x & 63) == 0) P.log_fill[lg_chunk] = lg_cur - lg_chunk * kLogChunk;

#if LT_WALK_BATCH && defined(LT_DIAG_MESH)
#if LT_WALK_BATCH == 2
    if (blockIdx.x == 7 && threadIdx.x == 0) {
        const double tot = (double)(clock64() - dg_clk_all);
        printf("[march diag] iterations %llu, cycles per iteration %.0f | alive %.1f, preparing %.1f | share of the wave's time: prepare %.3f, march round %.3f "
               "(in %.3f of iterations, %.1f lanes), drain %.3f (in %.3f of iterations, %.1f items), resolve %.3f, complete %.3f | complete %.1f lanes: "
               "boundary in %.3f of iterations (%.1f lanes), interaction in %.3f (%.1f lanes) | refills %.3f of iterations (%.1f lanes)\n",
               dg_iter, tot / dg_iter, (double)dg_alive / dg_iter, (double)dg_prep / dg_iter, dgm_clk[0] / tot, dgm_clk[1] / tot, (double)dg_trav_it / dg_iter,
               dg_trav_it ? (double)dg_trav / dg_trav_it : 0.0, dgm_clk[2] / tot, (double)dg_bvh_it / dg_iter, dg_bvh_it ? (double)dg_bvh / dg_bvh_it : 0.0,
               dgm_clk[3] / tot, dg_clk_bnd / tot, (double)dg_go / dg_iter, (double)dg_bnd_it / dg_iter, dg_bnd_it ? (double)dg_bnd / dg_bnd_it : 0.0,
               (double)dg_int_it / dg_iter, dg_int_it ? (double)dg_int / dg_int_it : 0.0, (double)dg_refill_it / dg_iter, dg_refill_it ? (double)dg_refill / dg_refill_it : 0.0);
    }
#else
    if (blockIdx.x == 7 && threadIdx.x == 0) {
        const double tot = (double)(clock64() - dg_clk_all);
        printf("[mesh diag] cycles per service %.0f; share of the wave's time: services %.3f, complete-stage %.3f; cycles per iteration %.0f\n",
               dg_trav_it ? (double)dg_clk_srv / dg_trav_it : 0.0, dg_clk_srv / tot, dg_clk_bnd / tot, tot / dg_iter);
    }
#endif
    if (blockIdx.x == 7 && threadIdx.x == 0)
        printf("[mesh diag] iterations %llu | alive %.1f/64 | prepare %.1f | waiting for a query %.1f | traversals: %.3f of iterations, %.1f lanes each | "
               "complete %.1f lanes: boundary in %.3f of iterations (%.1f lanes), interaction in %.3f (%.1f lanes) | refills: %.3f of iterations, %.1f lanes | "
               "services with BVH lanes %.3f of iterations (%.1f lanes), with 4-triangle lanes %.3f (%.1f lanes)\n",
               dg_iter, (double)dg_alive / dg_iter, (double)dg_prep / dg_iter, (double)dg_wait / dg_iter, (double)dg_trav_it / dg_iter,
               dg_trav_it ? (double)dg_trav / dg_trav_it : 0.0, (double)dg_go / dg_iter, (double)dg_bnd_it / dg_iter,
               dg_bnd_it ? (double)dg_bnd / dg_bnd_it : 0.0, (double)dg_int_it / dg_iter, dg_int_it ? (double)dg_int / dg_int_it : 0.0,
               (double)dg_refill_it / dg_iter, dg_refill_it ? (double)dg_refill / dg_refill_it : 0.0,
               (double)dg_bvh_it / dg_iter, dg_bvh_it ? (double)dg_bvh / dg_bvh_it : 0.0, (double)dg_l4_it / dg_iter, dg_l4_it ? (double)dg_l4 / dg_l4_it : 0.0);
#endif
    // ---------------- flush counters ----------------
    const double wa = wave_sum(acc_abs), wl = wave_sum(acc_lost);
    unsigned long long ws;
    if constexpr (kStepsScalar) ws = steps_w; else ws = wave_sum(acc_steps);
    if (lane == 0) {
        atomicAdd(&s_cnt[CW_ABSORBED], wa);
        atomicAdd(&s_cnt[CW_LOST], wl);
        __hip_atomic_fetch_add(&P.counters->steps, ws, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (LT_HAS_LOG)
        for (unsigned t = threadIdx.x; t < P.log_n_hist; t += blockDim.x)
            if (s_hist[t]) __hip_atomic_fetch_add(&P.log_hist[t * kLogGroups + (blockIdx.x & (kLogGroups - 1))], s_hist[t],
                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (kStepsScalar) if (threadIdx.x == 16 % blockDim.x) {      // the capped photons took no step: off the waves' counts (mod 2^64)
        const unsigned long long capped = *reinterpret_cast<const unsigned long long*>(lds_raw + LdsLayout<R>::kSlabCap);
        if (capped) __hip_atomic_fetch_add(&P.counters->steps, 0ull - capped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (PHASE != 2 && blockIdx.x == 0 && threadIdx.x == 8)      // (the tail's photons were counted by the bulk kernel)
        __hip_atomic_fetch_add(&P.counters->photons, P.n_photons, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x < 8)
        __hip_atomic_fetch_add(&P.counters->w[threadIdx.x], s_cnt[threadIdx.x], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}
#undef LT_HAS_LOG
#undef LT_STEP_ABSORB
#if LT_WALK_BATCH == 0
#undef LT_STEP_Y
#endif
#undef LT_STEP_DEP
#undef LT_STEP_HG
#undef LT_STEP_G
#if LT_INV_MODE == 2
#undef gx0
#undef gy0
#undef gz0
#undef ivx
#undef ivy
#undef ivz
#undef fnx
#undef fny
#undef fnz
#endif

