// lt_tallylabel.hip -- results by region: the voxel tally binned by a label volume (one byte per voxel) and by classes of the
// voxel's own value (lt_tally_label_sums, lt_tally_histogram).  Streaming passes over the grid and the label bytes that belong
// to it, HBM-bound, none with a global atomic:
//   k_label_bins     every voxel booked under (label, class of its value against ascending edges): voxels and weight per
//                    (label, class) in per-workgroup LDS bins with copies, the zero voxels per label beside them, the largest
//                    value per label; flushed once per workgroup into partial sums that k_sum_finish (lt_tallysum.hip) adds in
//                    a fixed order
//   k_label_reduce   the largest of the per-workgroup peaks (or the lowest of the per-workgroup indices) per label
//   k_label_argpeak  the lowest flat index at which a label holds its peak: only the workgroups whose own peak IS the label's
//                    read their part of the grid again -- in a traced grid a handful
// Label bytes: 0 .. n_labels - 1, or anything else (LT_LABEL_NONE) for a voxel that is left out.  Without a label volume every
// voxel has label 0.
#include <hip/hip_runtime.h>

#include "lt_tally.hpp"

namespace ltk {
namespace {

// 16 bytes of the grid: tested as two words, used as 16 / sizeof(T) elements
template <typename T> union alignas(16) Bits16 { u64 q[2]; T v[16 / sizeof(T)]; };
// the label bytes of one such group: 2 (f64, u64) or 4 (f32), aligned as the group is
template <int K> struct LabelWord { typedef uint16_t type; };
template <> struct LabelWord<4> { typedef uint32_t type; };

constexpr uint32_t kDepth = 4;                 // 16-byte groups a lane loads before it looks at any (k_stats_fold's chunks)
constexpr uint32_t kMaxCopies = 32;            // copies of every LDS bin; a lane adds to copy (lane & (copies - 1))
constexpr uint32_t kBinSlots = 1024;           // (label, class) bins x copies up to here (12 KiB), while a copy is left to halve
constexpr uint32_t kZeroSlots = 1024;          // labels x copies of the zero counters (4 KiB)
constexpr uint32_t kNoIndex = 0xffffffffu;

// the order of the values as unsigned integers: the raw integer, or the bits of a float that is >= 0
__device__ __forceinline__ u64 order_bits(u64 v) { return v; }
__device__ __forceinline__ u64 order_bits(double v) { return (u64)__double_as_longlong(v); }
__device__ __forceinline__ u64 order_bits(float v) { return (u64)__float_as_uint(v); }

struct LabelEdges { double e[kMaxStatEdges + 1]; };     // ascending, padded with NaN (never <= v) to 64

struct LabelShape {
    uint32_t n_labels, n_cls;       // n_cls = n_edges + 1
    uint32_t copies, zcopies;       // powers of two
    uint32_t want_peak;
};

template <bool LABELLED, int K>
__device__ __forceinline__ uint32_t label_of(typename LabelWord<K>::type w, int k)
{
    return LABELLED ? (uint32_t)(w >> (8 * k)) & 255u : 0u;
}

// LDS of a workgroup, in this order: edges f64 [64], weight A [bins x copies], peak u64 [n_labels], voxels u32 [bins x copies],
// zero voxels u32 [n_labels x zcopies].  A workgroup sees fewer than 2^21 voxels (the grid has fewer than 2^31, 2048 workgroups
// share it once it is large), so 32-bit counters hold; the partial sums are 64-bit.
// part_cnt / part_w [workgroup][label][class]: the NON-ZERO voxels and their weight; part_zero [workgroup][label]: the zero
// voxels, which the caller adds to the class of the value 0; part_peak [workgroup][label]: order_bits of the largest value.
// Most of a traced grid is zero and long runs of voxels share a label, so a lane counts zero voxels in a register for as long
// as the label stays the same (a 16-byte group of zeros under one label is one comparison), and every bin has `copies` copies.
template <typename T, bool LABELLED>
__global__ void __launch_bounds__(256) k_label_bins(const T* __restrict__ grid, const uint8_t* __restrict__ labels, size_t n, LabelEdges E,
                                                     LabelShape S, u64* __restrict__ part_cnt, typename AccOf<T>::type* __restrict__ part_w,
                                                     u64* __restrict__ part_zero, u64* __restrict__ part_peak)
{
    typedef typename AccOf<T>::type A;
    typedef typename LabelWord<16 / sizeof(T)>::type LW;
    constexpr int kV = 16 / sizeof(T);
    extern __shared__ double s_raw[];
    const uint32_t n_bins = S.n_labels * S.n_cls, n_slots = n_bins * S.copies, n_zslots = S.n_labels * S.zcopies;
    double* s_edge = s_raw;
    A* s_w = reinterpret_cast<A*>(s_edge + kMaxStatEdges + 1);
    u64* s_peak = reinterpret_cast<u64*>(s_w + n_slots);
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_peak + S.n_labels);
    uint32_t* s_zero = s_cnt + n_slots;
    if (threadIdx.x <= kMaxStatEdges) s_edge[threadIdx.x] = E.e[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < n_slots; i += 256) { s_cnt[i] = 0; s_w[i] = 0; }
    for (uint32_t i = threadIdx.x; i < n_zslots; i += 256) s_zero[i] = 0;
    for (uint32_t i = threadIdx.x; i < S.n_labels; i += 256) s_peak[i] = 0;
    __syncthreads();
    const uint32_t copy = threadIdx.x & (S.copies - 1), zcopy = threadIdx.x & (S.zcopies - 1);
    const bool classed = S.n_cls > 1;
    uint32_t z_label = 0, z_count = 0;              // the run of zero voxels this lane is in
    auto zeros = [&](uint32_t l, uint32_t count) {
        if (l >= S.n_labels) return;
        if (l != z_label) {
            if (z_count) atomicAdd(&s_zero[z_label * S.zcopies + zcopy], z_count);
            z_label = l; z_count = 0;
        }
        z_count += count;
    };
    auto book = [&](uint32_t l, T s1) {
        if (l >= S.n_labels) return;
        uint32_t c = 0;
        if (classed) {
            const double v = as_weight(s1);
#pragma unroll
            for (uint32_t step = (kMaxStatEdges + 1) / 2; step; step >>= 1)
                if (s_edge[c + step - 1] <= v) c += step;
        }
        const uint32_t slot = (l * S.n_cls + c) * S.copies + copy;
        atomicAdd(&s_cnt[slot], 1u);
        lds_add(&s_w[slot], (A)s1);
        if (S.want_peak) {
            const u64 b = order_bits(s1);
            if (b > s_peak[l]) atomicMax(&s_peak[l], b);
        }
    };
    const size_t nvec = n / kV, stride = (size_t)gridDim.x * 256;
    const Bits16<T>* pg = reinterpret_cast<const Bits16<T>*>(grid);
    const LW* pl = reinterpret_cast<const LW*>(labels);
    for (size_t i0 = (size_t)blockIdx.x * (256 * kDepth) + threadIdx.x; i0 < nvec; i0 += stride * kDepth) {
        Bits16<T> g[kDepth];
        LW w[kDepth];
#pragma unroll
        for (uint32_t u = 0; u < kDepth; u++) {
            const size_t i = i0 + u * 256;
            w[u] = 0;
            if (i < nvec) { g[u] = pg[i]; if (LABELLED) w[u] = pl[i]; }
            else g[u].q[0] = g[u].q[1] = 0;
        }
#pragma unroll
        for (uint32_t u = 0; u < kDepth; u++) {
            if (i0 + u * 256 >= nvec) continue;
            const uint32_t l0 = label_of<LABELLED, kV>(w[u], 0);
            bool same = true;
#pragma unroll
            for (int k = 1; k < kV; k++) same = same && label_of<LABELLED, kV>(w[u], k) == l0;
            if ((g[u].q[0] | g[u].q[1]) == 0 && same) { zeros(l0, kV); continue; }
#pragma unroll
            for (int k = 0; k < kV; k++) {
                const uint32_t l = label_of<LABELLED, kV>(w[u], k);
                if (g[u].v[k] == (T)0) zeros(l, 1);
                else book(l, g[u].v[k]);
            }
        }
    }
    const size_t t = nvec * kV + threadIdx.x;       // the last n % kV voxels go one by one
    if (blockIdx.x == 0 && t < n) {
        const uint32_t l = LABELLED ? labels[t] : 0u;
        const T s1 = grid[t];
        if (s1 == (T)0) zeros(l, 1);
        else book(l, s1);
    }
    if (z_count) atomicAdd(&s_zero[z_label * S.zcopies + zcopy], z_count);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < n_bins; b += 256) {
        u64 cnt = 0;
        A w = 0;
        for (uint32_t k = 0; k < S.copies; k++) { cnt += s_cnt[b * S.copies + k]; w += s_w[b * S.copies + k]; }
        part_cnt[(size_t)blockIdx.x * n_bins + b] = cnt;
        part_w[(size_t)blockIdx.x * n_bins + b] = w;
    }
    for (uint32_t l = threadIdx.x; l < S.n_labels; l += 256) {
        u64 z = 0;
        for (uint32_t k = 0; k < S.zcopies; k++) z += s_zero[l * S.zcopies + k];
        part_zero[(size_t)blockIdx.x * S.n_labels + l] = z;
        part_peak[(size_t)blockIdx.x * S.n_labels + l] = s_peak[l];
    }
}

// out[l] = the largest (MAX) or the smallest of part[0][l] .. part[P - 1][l]: one wave per label
template <typename V, bool MAX>
__global__ void __launch_bounds__(64) k_label_reduce(const V* __restrict__ part, uint32_t P, uint32_t n_labels, V* __restrict__ out)
{
    const uint32_t l = blockIdx.x;
    V acc = MAX ? (V)0 : (V)~(V)0;
    for (uint32_t p = threadIdx.x; p < P; p += 64) {
        const V v = part[(size_t)p * n_labels + l];
        acc = MAX ? (v > acc ? v : acc) : (v < acc ? v : acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const V v = __shfl_down(acc, o, 64);
        acc = MAX ? (v > acc ? v : acc) : (v < acc ? v : acc);
    }
    if (threadIdx.x == 0) out[l] = acc;
}

// part_idx [workgroup][label]: the lowest flat index among the workgroup's voxels of the label that hold peak[label], kNoIndex
// if there is none.  Launched with k_label_bins' grid, so that workgroup b reads what it read there: if none of its own peaks
// (part_peak[b]) is a label's peak it is done without a load.  A label whose peak is 0 is not looked for (every voxel of it holds
// the peak: the first one is known to the host).
template <typename T, bool LABELLED>
__global__ void __launch_bounds__(256) k_label_argpeak(const T* __restrict__ grid, const uint8_t* __restrict__ labels, size_t n,
                                                        uint32_t n_labels, const u64* __restrict__ peak, const u64* __restrict__ part_peak,
                                                        uint32_t* __restrict__ part_idx)
{
    typedef typename LabelWord<16 / sizeof(T)>::type LW;
    constexpr int kV = 16 / sizeof(T);
    __shared__ u64 s_peak[64];
    __shared__ uint32_t s_idx[64];
    __shared__ uint32_t s_any;
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    bool mine = false;           // thread l: is this workgroup's peak of label l the label's?
    if (threadIdx.x < n_labels) {
        const u64 p = peak[threadIdx.x];
        mine = p != 0 && part_peak[(size_t)blockIdx.x * n_labels + threadIdx.x] == p;
        s_peak[threadIdx.x] = p;
        s_idx[threadIdx.x] = mine ? kNoIndex : 0u;       // (0: no index is below it, the label is not looked for)
        if (mine) s_any = 1;
    }
    __syncthreads();
    if (s_any) {
        auto look = [&](uint32_t l, T s1, size_t idx) {
            if (l >= n_labels) return;
            if (order_bits(s1) == s_peak[l] && (uint32_t)idx < s_idx[l]) atomicMin(&s_idx[l], (uint32_t)idx);
        };
        const size_t nvec = n / kV, stride = (size_t)gridDim.x * 256;
        const Bits16<T>* pg = reinterpret_cast<const Bits16<T>*>(grid);
        const LW* pl = reinterpret_cast<const LW*>(labels);
        for (size_t i0 = (size_t)blockIdx.x * (256 * kDepth) + threadIdx.x; i0 < nvec; i0 += stride * kDepth) {
            Bits16<T> g[kDepth];
#pragma unroll
            for (uint32_t u = 0; u < kDepth; u++) {
                const size_t i = i0 + u * 256;
                if (i < nvec) g[u] = pg[i];
                else g[u].q[0] = g[u].q[1] = 0;
            }
#pragma unroll
            for (uint32_t u = 0; u < kDepth; u++) {
                if ((g[u].q[0] | g[u].q[1]) == 0) continue;      // (a group past the end is zero)
                const size_t i = i0 + u * 256;
                const LW w = LABELLED ? pl[i] : (LW)0;
#pragma unroll
                for (int k = 0; k < kV; k++) look(label_of<LABELLED, kV>(w, k), g[u].v[k], i * kV + k);
            }
        }
        const size_t t = nvec * kV + threadIdx.x;
        if (blockIdx.x == 0 && t < n) look(LABELLED ? labels[t] : 0u, grid[t], t);
    }
    __syncthreads();
    if (threadIdx.x < n_labels) part_idx[(size_t)blockIdx.x * n_labels + threadIdx.x] = mine ? s_idx[threadIdx.x] : kNoIndex;
}

uint32_t pow2_floor(uint32_t v) { uint32_t p = 1; while (p * 2 <= v) p *= 2; return p; }

LabelShape label_shape(int n_labels, int n_edges, bool want_peak)
{
    LabelShape S;
    S.n_labels = (uint32_t)n_labels; S.n_cls = (uint32_t)n_edges + 1;
    const uint32_t bins = S.n_labels * S.n_cls;
    S.copies = bins >= kBinSlots ? 1 : pow2_floor(kBinSlots / bins);
    if (S.copies > kMaxCopies) S.copies = kMaxCopies;
    S.zcopies = pow2_floor(kZeroSlots / S.n_labels);
    if (S.zcopies > kMaxCopies) S.zcopies = kMaxCopies;
    S.want_peak = want_peak;
    return S;
}

size_t label_lds_bytes(const LabelShape& S)
{
    const size_t slots = (size_t)S.n_labels * S.n_cls * S.copies;
    return (kMaxStatEdges + 1) * 8 + slots * 12 + (size_t)S.n_labels * 8 + (size_t)S.n_labels * S.zcopies * 4;
}

}  // namespace

uint32_t tally_label_parts(size_t n_vox, int tally) { return blocks_for(n_vox, (size_t)256 * kDepth * (16 / tally_elem_bytes(tally))); }

size_t tally_label_partial_bytes(size_t n_vox, int tally, int n_labels, int n_edges)
{
    const size_t P = tally_label_parts(n_vox, tally), bins = (size_t)n_labels * ((size_t)n_edges + 1);
    return P * (bins * 16 + (size_t)n_labels * 24);
}

hipError_t launch_tally_label_bins(const void* grid, const uint8_t* labels, int tally, size_t n, int n_labels, const double* edges,
                                   int n_edges, int want_peak, void* partials, double* out, hipStream_t s)
{
    const LabelShape S = label_shape(n_labels, n_edges, want_peak != 0);
    const uint32_t P = tally_label_parts(n, tally);
    const size_t bins = (size_t)S.n_labels * S.n_cls, L = S.n_labels;
    LabelEdges E;
    for (int i = 0; i <= kMaxStatEdges; i++) E.e[i] = i < n_edges ? edges[i] : __builtin_nan("");
    u64* part_cnt = (u64*)partials;
    u64* part_w = part_cnt + P * bins;          // (A is 8 bytes wide whatever the tally)
    u64* part_zero = part_w + P * bins;
    u64* part_peak = part_zero + P * L;
    uint32_t* part_idx = (uint32_t*)(part_peak + P * L);
    const size_t lds = label_lds_bytes(S);
    with_tally_type(tally, [&](auto t) {
        typedef decltype(t) T;
        typedef typename AccOf<T>::type A;
        if (labels)
            hipLaunchKernelGGL((k_label_bins<T, true>), dim3(P), dim3(256), lds, s, (const T*)grid, labels, n, E, S, part_cnt, (A*)part_w, part_zero, part_peak);
        else
            hipLaunchKernelGGL((k_label_bins<T, false>), dim3(P), dim3(256), lds, s, (const T*)grid, labels, n, E, S, part_cnt, (A*)part_w, part_zero, part_peak);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // out, 8-byte words: weight f64 [bins], raw weight u64 [bins] (u64 fixed point only), voxels u64 [bins], zero voxels u64
    // [labels], peak bits u64 [labels], peak index u32 [labels] (padded to words); two more blocks take the f64 forms nobody reads
    const bool fx = tally == LT_TALLY_U64FX;
    u64* raw = (u64*)out;
    double* unused = out + 3 * bins + 3 * L;
    e = launch_tally_sum_finish(part_w, fx, P, bins, out, fx ? raw + bins : nullptr, s);
    if (e != hipSuccess) return e;
    e = launch_tally_sum_finish(part_cnt, 1, P, bins, unused, raw + 2 * bins, s);
    if (e != hipSuccess) return e;
    e = launch_tally_sum_finish(part_zero, 1, P, L, unused, raw + 3 * bins, s);
    if (e != hipSuccess || !want_peak) return e;
    u64* peak = raw + 3 * bins + L;
    uint32_t* peak_idx = (uint32_t*)(peak + L);
    hipLaunchKernelGGL((k_label_reduce<u64, true>), dim3(S.n_labels), dim3(64), 0, s, part_peak, P, S.n_labels, peak);
    with_tally_type(tally, [&](auto t) {
        typedef decltype(t) T;
        if (labels)
            hipLaunchKernelGGL((k_label_argpeak<T, true>), dim3(P), dim3(256), 0, s, (const T*)grid, labels, n, S.n_labels, peak, part_peak, part_idx);
        else
            hipLaunchKernelGGL((k_label_argpeak<T, false>), dim3(P), dim3(256), 0, s, (const T*)grid, labels, n, S.n_labels, peak, part_peak, part_idx);
    });
    hipLaunchKernelGGL((k_label_reduce<uint32_t, false>), dim3(S.n_labels), dim3(64), 0, s, part_idx, P, S.n_labels, peak_idx);
    return hipGetLastError();
}

size_t tally_label_out_bytes(int n_labels, int n_edges)
{
    const size_t bins = (size_t)n_labels * ((size_t)n_edges + 1), L = (size_t)n_labels;
    return (3 * bins + 3 * L + bins) * 8;       // the results (the 32-bit indices in L words) and the block nobody reads
}

}  // namespace ltk
