// lt_tally.hpp -- the tally's three element types (f32 / f64 / u64 fixed point) in one place, for the walk (lt_walk.hip), the log
// reduction (lt_logtally.hip), the whole-grid passes (lt_tallysum.hip), the batch statistics (lt_tallystats.hip) and the box
// read-out (lt_tallybox.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "lt_internal.hpp"

namespace ltk {

typedef unsigned long long u64;

// element type of a tally code (LT_TALLY_NONE, the walk without deposition: double)
template <int TALLY> struct TallyT { typedef double type; };
template <> struct TallyT<LT_TALLY_F32> { typedef float type; };
template <> struct TallyT<LT_TALLY_U64FX> { typedef u64 type; };
// type that elements of type T are summed in: u64 for the fixed-point tally (integer sums: exact, any order), f64 for the f32 and
// f64 tallies (in LDS ds_add_f64 sustains twice the rate of ds_add_f32, and an f32 grid sees one rounding per tile, not per deposit)
template <typename T> struct AccOf { typedef double type; };
template <> struct AccOf<u64> { typedef u64 type; };
// an element, or a sum of elements, as weight: the units of lt_read_grid_f64
__device__ __forceinline__ double as_weight(u64 v) { return (double)v * (1.0 / LT_FX_SCALE); }
__device__ __forceinline__ double as_weight(double v) { return v; }
__device__ __forceinline__ double as_weight(float v) { return (double)v; }
template <typename A> __device__ __forceinline__ void lds_add(A* p, A v) { atomicAdd(p, v); }
template <typename T> struct alignas(16) Vec16 { T v[16 / sizeof(T)]; };           // an aligned 16-byte load of elements

inline size_t tally_elem_bytes(int tally) { return tally == LT_TALLY_F32 ? 4 : 8; }
// grid of a streaming pass: one workgroup per items_per_block items up to kMaxBlocks (256 CUs x 8 resident workgroups), then grid-strided
constexpr uint32_t kMaxBlocks = 2048;
inline uint32_t blocks_for(size_t n_items, size_t items_per_block)
{
    const size_t b = (n_items + items_per_block - 1) / items_per_block;
    return (uint32_t)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}
// f(T{}) with T the element type of `tally`: the one place where a run-time tally code picks a template instantiation
template <typename F> inline auto with_tally_type(int tally, F&& f)
{
    if (tally == LT_TALLY_F32) return f(float{});
    if (tally == LT_TALLY_F64) return f(double{});
    return f(u64{});
}

}  // namespace ltk
