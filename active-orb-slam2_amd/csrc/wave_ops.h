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
// the same move for a double, two 32-bit moves.  `old` (the value of lanes without a source) is 0 with bound_ctrl: every lane has
// a source under the words this header uses with it, so it is never read -- and with `v` there the compiler copied both halves
// with a plain v_mov_b32 in front of every DPP move (the destination is tied to `old`)
template <int kCtrl>
__device__ __forceinline__ double dpp_f64(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, kCtrl, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), kCtrl, 0xf, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// lanes of the banks in kBanks (bank q = the quad of lanes 4 q .. 4 q + 3 of every row): v of the lane kCtrl names; the other
// lanes: `old`.  The enabled lanes must have a source under kCtrl.
template <int kCtrl, int kBanks>
__device__ __forceinline__ double dpp_f64_banks(double old, double v)
{
    const long long o = __double_as_longlong(old), b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp((int)o, (int)b, kCtrl, 0xf, kBanks, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(b >> 32), kCtrl, 0xf, kBanks, false);
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

// Sum of N doubles per thread over a workgroup of NT threads (all active; part: NT / 16 * N doubles of LDS), the result in every
// thread.  Row sums by DPP (lane 0 of a row of 16 is the one that is kept), then every thread adds the row partials in row order:
// the order depends on nothing but the thread number.  The second barrier lets `part` be written again.
template <int N, int NT = 256>
__device__ __forceinline__ void block_sum_f64(double (&v)[N], double *part)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = row_sum_f64(v[i]);
    if ((tid & 15) == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) part[(tid >> 4) * N + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = part[i];
        for (int r = 1; r < NT / 16; ++r) s += part[r * N + i];
        v[i] = s;
    }
    __syncthreads();
}
// the same for one value
template <int NT = 256>
__device__ __forceinline__ double block_sum_f64(double v, double *part)
{
    double a[1] = {v};
    block_sum_f64<1, NT>(a, part);
    return a[0];
}

// ---- K row sums at once as a reduce-scatter: the totals of row_sum_f64 (the same operands in the same tree, so the same bits)
// without forming every total in every lane.  The four levels pair lane ^ 1, lane ^ 2, lane ^ 4, lane ^ 8; at a level a lane keeps
// one value of each pair of its remaining values and hands the other one to its partner, who adds it to the one it kept:
// n values become ceil(n / 2) (an unpaired last value is added the butterfly's way), and after the fourth level the total of
// every value sits in slot s of the lanes row_scatter_index names.  IEEE addition is commutative, so which of the two lanes
// adds does not show in the bits.
constexpr int row_scatter_count(int K, int level) { return level == 0 ? K : ((K + (1 << level) - 1) >> level); }
// slots a lane holds after row_sums_scatter_f64<K>
constexpr int row_scatter_slots(int K) { return row_scatter_count(K, 4); }
// the value whose total slot s of lane li of a row (li = lane & 15) holds afterwards.  Every value has a (li, s); the totals of
// values that were unpaired at some level sit in several lanes (the same bits in each).
template <int K>
__host__ __device__ constexpr int row_scatter_index(int s, int li)
{
    constexpr int n0 = K, n1 = row_scatter_count(K, 1), n2 = row_scatter_count(K, 2), n3 = row_scatter_count(K, 3);   // values before a level
    int idx = s;
    idx = ((n3 & 1) && idx == n3 / 2) ? n3 - 1 : 2 * idx + ((li >> 3) & 1);
    idx = ((n2 & 1) && idx == n2 / 2) ? n2 - 1 : 2 * idx + ((li >> 2) & 1);
    idx = ((n1 & 1) && idx == n1 / 2) ? n1 - 1 : 2 * idx + ((li >> 1) & 1);
    idx = ((n0 & 1) && idx == n0 / 2) ? n0 - 1 : 2 * idx + (li & 1);
    return idx;
}
// the first (li, s) that holds value i
template <int K>
__host__ __device__ constexpr void row_scatter_owner(int i, int &li, int &s)
{
    for (li = 0; li < 16; ++li)
        for (s = 0; s < row_scatter_slots(K); ++s)
            if (row_scatter_index<K>(s, li) == i) return;
}

// one pair of a level with partner lane ^ 1 / lane ^ 2: `up` = the lane's bit of the level
template <int kCtrl>
__device__ __forceinline__ double row_scatter_pair_quad(double a, double b, bool up)
{
    const double keep = up ? b : a, send = up ? a : b;
    return keep + dpp_f64<kCtrl>(send);
}
// one pair of a level with partner lane ^ 4 / lane ^ 8: a bank is a quad, so the bank mask selects between the lane's own value
// and the partner's.  kLo = the banks whose bit of the level is 0; they take a from kFromUp, the others b from kFromLo
template <int kFromUp, int kFromLo, int kLo>
__device__ __forceinline__ double row_scatter_pair_banks(double a, double b)
{
    const double x = dpp_f64_banks<kFromLo, 0xf & ~kLo>(a, b);   // lower lanes: own a; upper lanes: the partner's b
    const double y = dpp_f64_banks<kFromUp, kLo>(b, a);          // lower lanes: the partner's a; upper lanes: own b
    return x + y;
}
// v + v of lane ^ 4 (values that differ between the lanes of a quad: row_half_mirror would not do)
__device__ __forceinline__ double row_scatter_single_4(double v)
{
    return v + dpp_f64_banks<0x114, 0xa>(dpp_f64_banks<0x104, 0x5>(v, v), v);   // row_shl:4 into banks 0, 2; row_shr:4 into banks 1, 3
}

template <int K, int N>
__device__ __forceinline__ void row_sums_scatter_f64(double (&v)[N])   // v[0 .. K) -> v[0 .. row_scatter_slots(K))
{
    static_assert(K >= 1 && K <= N, "K values of the array");
    const int lane = threadIdx.x & 15;
    constexpr int n0 = K, n1 = row_scatter_count(K, 1), n2 = row_scatter_count(K, 2), n3 = row_scatter_count(K, 3);
    const bool up0 = lane & 1, up1 = lane & 2;
#pragma unroll
    for (int m = 0; m < n0 / 2; ++m) v[m] = row_scatter_pair_quad<0xB1>(v[2 * m], v[2 * m + 1], up0);
    if (n0 & 1) v[n0 / 2] = v[n0 - 1] + dpp_f64<0xB1>(v[n0 - 1]);
#pragma unroll
    for (int m = 0; m < n1 / 2; ++m) v[m] = row_scatter_pair_quad<0x4E>(v[2 * m], v[2 * m + 1], up1);
    if (n1 & 1) v[n1 / 2] = v[n1 - 1] + dpp_f64<0x4E>(v[n1 - 1]);
#pragma unroll
    for (int m = 0; m < n2 / 2; ++m) v[m] = row_scatter_pair_banks<0x104, 0x114, 0x5>(v[2 * m], v[2 * m + 1]);   // row_shl:4, row_shr:4
    if (n2 & 1) v[n2 / 2] = row_scatter_single_4(v[n2 - 1]);
#pragma unroll
    for (int m = 0; m < n3 / 2; ++m) v[m] = row_scatter_pair_banks<0x128, 0x128, 0x3>(v[2 * m], v[2 * m + 1]);   // row_ror:8 = lane ^ 8
    if (n3 & 1) v[n3 / 2] = v[n3 - 1] + dpp_f64<0x128>(v[n3 - 1]);
}
// the totals into out[i], i = the value's index (LDS or memory; lanes that hold the same total write the same bits)
template <int K, int N, int S = 0>
__device__ __forceinline__ void row_scatter_store(const double (&v)[N], double *out)
{
    if constexpr (S < row_scatter_slots(K)) {   // (a slot per instantiation: v is indexed by constants only and stays in registers)
        out[row_scatter_index<K>(S, threadIdx.x & 15)] = v[S];
        row_scatter_store<K, N, S + 1>(v, out);
    }
}

// ---- groups of 8 lanes (group g = lanes 8 g .. 8 g + 7, half a row; li = lane & 7)
// v of the lane in front (lane - 1): row_shr:1.  Lane 0 of a row has no source and gets 0; li == 0 never uses what it gets.
__device__ __forceinline__ float group8_prev(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));
}
__device__ __forceinline__ double group8_prev(double v) { return dpp_f64<0x111>(v); }
// v of lane 7 of the group in every lane of the group: quad_perm [3,3,3,3] puts lane 3 / lane 7 into every lane of its quad, then
// row_shl:4 into banks 0 and 2 hands the upper quad's value to the lower one
__device__ __forceinline__ int group8_last_i32(int v)
{
    const int q = __builtin_amdgcn_update_dpp(0, v, 0xFF, 0xf, 0xf, true);
    return __builtin_amdgcn_update_dpp(q, q, 0x104, 0xf, 0x5, false);
}
__device__ __forceinline__ float group8_last(float v) { return __int_as_float(group8_last_i32(__float_as_int(v))); }
__device__ __forceinline__ double group8_last(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = group8_last_i32((int)b), hi = group8_last_i32((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// The ORDERED sum of a group: ((carry + v of lane 0) + v of lane 1) + ... over the first min(cnt, 8) lanes of the group, one add
// after the other in lane order -- no tree, so the bits are those of a serial loop over the lanes.  carry and cnt are the same in
// every lane of a group; the result is too.  The partial sum walks up the group: at step k lane k takes it from lane k - 1 and adds
// its own value (or hands it on unchanged behind the count).  T = float or double.
template <class T>
__device__ __forceinline__ T group8_sum_ordered(T carry, T v, int cnt)
{
    const int li = threadIdx.x & 7;
    T s = (li == 0 && cnt > 0) ? carry + v : carry;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const T t = group8_prev(s);
        s = li == k ? (k < cnt ? t + v : t) : s;
    }
    return group8_last(s);
}
// every lane: the max over its group of 8
__device__ __forceinline__ int group8_max_i32(int v)
{
    v = max(v, dpp_i32<0xB1>(v));
    v = max(v, dpp_i32<0x4E>(v));
    v = max(v, dpp_i32<0x141>(v));
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

// Sum of one int per WAVE (wave_value: wave-uniform) over a workgroup of NT threads (all active; part: NT / 64 ints of LDS), the
// result in every thread.  Two barriers inside: one in front of the stores, so `part` may have been read until the call (by the
// previous call with the same part included), one behind them.
template <int NT>
__device__ __forceinline__ int block_sum_waves_i32(int wave_value, int32_t *part)
{
    static_assert(NT % 64 == 0, "whole waves");
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = wave_value;
    __syncthreads();
    int s = part[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) s += part[w];
    return s;
}
// Sum of one int per thread over a workgroup of NT threads: the same, with the same two barriers, on the waves' sums.
template <int NT>
__device__ __forceinline__ int block_sum_i32(int v, int32_t *part)
{
    return block_sum_waves_i32<NT>(wave_sum_i32(v), part);
}

}  // namespace aos2
