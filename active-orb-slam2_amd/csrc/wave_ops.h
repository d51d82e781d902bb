// Wave64 cross-lane primitives on DPP for gfx950 (no LDS round trips): the only definition of the DPP moves, the row /
// wave reductions and the scans that the kernels use.  HIP's __shfl_xor / __shfl_up compile to ds_bpermute_b32, i.e. one
// dependent LDS access per step; these helpers use row-level DPP steps and v_readlane.
// ALL 64 LANES MUST BE ACTIVE AT THE CALL (a DPP step reads registers of other lanes whatever the exec mask says, and the
// readlanes of the wave forms read lanes 0 / 16 / 32 / 48): call them from wave-uniform control flow only.
#pragma once
#include <hip/hip_runtime.h>

namespace aos2 {

// v of another lane of the same row of 16 (a row = lanes 16 r .. 16 r + 15).  The xor butterfly over a row is the four steps
//   0xB1  quad_perm [1,0,3,2]  lane ^ 1        0x141 row_half_mirror  lane ^ 7  (8 lanes reversed)
//   0x4E  quad_perm [2,3,0,1]  lane ^ 2        0x140 row_mirror       lane ^ 15 (16 lanes reversed)
// after which every lane of the row has combined all 16 values.  Every lane has a source under these four words.
template <int kCtrl>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, kCtrl, 0xf, 0xf, false);
}
// the same move for an operand of a signed add / max: with 0 as the value of lanes without a source (there are none) the
// compiler folds the move into the instruction (v_add_u32_dpp, v_max_i32_dpp); with `v` there it keeps a v_mov_b32_dpp
template <int kCtrl>
__device__ __forceinline__ int dpp_i32(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, kCtrl, 0xf, 0xf, false);
}
template <int kCtrl>
__device__ __forceinline__ double dpp_f64(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp((int)b, (int)b, kCtrl, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(b >> 32), (int)(b >> 32), kCtrl, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// value of `v` in lane `src` (wave-uniform index), uniform result
__device__ __forceinline__ double readlane_f64(double v, int src)
{
    const long long bits = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(bits & 0xffffffffll), src);
    const int hi = __builtin_amdgcn_readlane((int)(bits >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ int wave_row_sum_i32(int v)   // every lane: the sum of its row of 16 lanes
{
    v += dpp_i32<0xB1>(v);
    v += dpp_i32<0x4E>(v);
    v += dpp_i32<0x141>(v);
    v += dpp_i32<0x140>(v);
    return v;
}

__device__ __forceinline__ int wave_sum_i32(int v)       // wave-uniform sum of the 64 lanes
{
    v = wave_row_sum_i32(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}

__device__ __forceinline__ int wave_max_i32(int v)       // wave-uniform max of the 64 lanes; v >= 0
{
    v = max(v, dpp_i32<0xB1>(v));
    v = max(v, dpp_i32<0x4E>(v));
    v = max(v, dpp_i32<0x141>(v));
    v = max(v, dpp_i32<0x140>(v));
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

__device__ __forceinline__ uint32_t wave_row_min_u32(uint32_t k)  // every lane: the min of its row of 16 lanes
{
    k = min(k, dpp_u32<0xB1>(k));
    k = min(k, dpp_u32<0x4E>(k));
    k = min(k, dpp_u32<0x141>(k));
    k = min(k, dpp_u32<0x140>(k));
    return k;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t k)      // wave-uniform min of the 64 lanes
{
    k = wave_row_min_u32(k);
    uint32_t a = __builtin_amdgcn_readlane(k, 0);
    a = min(a, (uint32_t)__builtin_amdgcn_readlane(k, 16));
    a = min(a, (uint32_t)__builtin_amdgcn_readlane(k, 32));
    a = min(a, (uint32_t)__builtin_amdgcn_readlane(k, 48));
    return a;
}

// Sum of `v` over the 16 lanes of a row: VALU speed, no LDS.  Every lane of the row ends with the row's total (lanes may
// differ in the last bit: the butterfly adds in a lane-dependent order; callers read one fixed lane per row).
__device__ __forceinline__ double row_sum_f64(double v)
{
    v += dpp_f64<0xB1>(v);
    v += dpp_f64<0x4E>(v);
    v += dpp_f64<0x141>(v);
    v += dpp_f64<0x140>(v);
    return v;
}

__device__ __forceinline__ int wave_incl_scan_i32(int v)  // inclusive prefix sum over the lanes
{
    int x = v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);   // row_shr:1 (lanes without a source add 0)
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);   // row_shr:8  -> inclusive scan inside each row
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2 and 3
    return x;
}

// Exclusive prefix sum of one int per thread over a workgroup of NT threads (all active; wsum: NT / 64 ints of LDS);
// `total` = the workgroup's sum, in every thread.  One barrier inside; the caller needs another one before wsum is written
// again (the next call with the same wsum included).
template <int NT>
__device__ __forceinline__ int block_excl_scan_i32(int v, int32_t *wsum, int &total)
{
    static_assert(NT % 64 == 0, "whole waves");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan_i32(v);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int excl = incl - v;
    total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        if (w == wave) excl += total;
        total += wsum[w];
    }
    return excl;
}

}  // namespace aos2
