// The arrays of the map that an aos2_local_map handle keeps resident: the covisibility graph of Tracking::UpdateLocalMap (11
// arrays) and the view of LocalMapping::KeyFrameCulling (6 arrays, parallel to the graph's).  ONE list of them -- lm_each -- with
// their lengths and the value of an appended row; the device block, the host mirror, the delta of aos2_local_map_apply and every
// copy between them are passes over that list.  No HIP runtime calls: host C++ and kernels.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "regions.h"

namespace aos2 {

constexpr int kLmNeighbours = 10;   // GetBestCovisibilityKeyFrames(10)

template <class T>
using LmPtr = const T *;   // device or host addresses
template <class T>
using LmVec = std::vector<T>;   // the handle's mirror

// A delta carries the same arrays over its named rows only: offsets over those rows, entries of those rows.
template <template <class> class F>
struct LmArrays {
    F<uint8_t> point_bad;
    F<int32_t> point_nobs, obs_off, obs_kf;
    F<uint8_t> kf_bad;
    F<int32_t> kf_mp_off, kf_mp, kf_best, kf_child_off, kf_child, kf_parent;
    // the culling view (pointers: NULL without one)
    F<int32_t> obs_idx;
    F<int8_t> kf_octave;
    F<float> kf_depth;
    F<uint8_t> kf_stereo;
    F<float> kf_th_depth;
    F<uint8_t> kf_flags;
};

// What the kernels of csrc/local_map.hip and csrc/kf_culling.hip take.  The counts stand IN FRONT of the pointers, where the
// kernels' first scalar loads find them: behind the 17 pointers, aos2_frames_update_local_map of one frame measured 6 % slower
// (profiles/README.md).
struct LmGraphCounts {
    int n_points, n_kfs;
};
struct LmGraph : LmGraphCounts, LmArrays<LmPtr> {
};

// Three row sets, and the entries of the CSR array over each.  The graph: (n_points, n_kfs, n_kfs, n_obs, n_mp, n_child); a
// delta: its named point / match / link rows and the entries they carry.
struct LmCounts {
    size_t point_rows, match_rows, link_rows, obs, mp, child;
};

// an array's length; the classes of one row set are adjacent (lm_row_set)
enum LmLen { kLmPerPoint, kLmPointOff, kLmPerObs, kLmMatchOff, kLmPerMatch, kLmPerLink, kLmLinkNb, kLmLinkOff, kLmPerChild };
inline size_t lm_len(const LmCounts &c, LmLen l)
{
    const size_t len[] = {c.point_rows, c.point_rows + 1, c.obs, c.match_rows + 1, c.mp, c.link_rows, c.link_rows * kLmNeighbours,
                          c.link_rows + 1, c.child};
    return len[l];
}
inline int lm_row_set(LmLen l) { return l < kLmMatchOff ? 0 : l < kLmPerLink ? 1 : 2; }   // point, match, link rows
inline size_t lm_rows(const LmCounts &c, int row_set) { return row_set == 0 ? c.point_rows : row_set == 1 ? c.match_rows : c.link_rows; }

// an appended row that a delta does not name: the empty slot of the table
namespace lm_fill {
constexpr uint8_t point_bad = 1, kf_bad = 1, kf_flags = 0;
constexpr int32_t point_nobs = 0, kf_best = -1, kf_parent = -1;
constexpr float kf_th_depth = 0.f;
}  // namespace lm_fill

// THE list: fn(member of a, member of b, length class, fill) once per array, in the order of the resident block -- the graph,
// then the view.  a and b need only have members of these names (the public structs of include/aos2.h do).
template <class A, class B, class Fn>
inline void lm_each_graph(A &a, B &b, Fn &&fn)
{
    fn(a.point_bad, b.point_bad, kLmPerPoint, lm_fill::point_bad);
    fn(a.kf_bad, b.kf_bad, kLmPerLink, lm_fill::kf_bad);
    fn(a.point_nobs, b.point_nobs, kLmPerPoint, lm_fill::point_nobs);
    fn(a.obs_off, b.obs_off, kLmPointOff, int32_t(0));
    fn(a.obs_kf, b.obs_kf, kLmPerObs, int32_t(0));
    fn(a.kf_mp_off, b.kf_mp_off, kLmMatchOff, int32_t(0));
    fn(a.kf_mp, b.kf_mp, kLmPerMatch, int32_t(0));
    fn(a.kf_best, b.kf_best, kLmLinkNb, lm_fill::kf_best);
    fn(a.kf_child_off, b.kf_child_off, kLmLinkOff, int32_t(0));
    fn(a.kf_child, b.kf_child, kLmPerChild, int32_t(0));
    fn(a.kf_parent, b.kf_parent, kLmPerLink, lm_fill::kf_parent);
}
template <class A, class B, class Fn>
inline void lm_each_view(A &a, B &b, Fn &&fn)
{
    fn(a.obs_idx, b.obs_idx, kLmPerObs, int32_t(0));
    fn(a.kf_octave, b.kf_octave, kLmPerMatch, int8_t(0));
    fn(a.kf_depth, b.kf_depth, kLmPerMatch, 0.f);
    fn(a.kf_stereo, b.kf_stereo, kLmPerMatch, uint8_t(0));
    fn(a.kf_th_depth, b.kf_th_depth, kLmPerLink, lm_fill::kf_th_depth);
    fn(a.kf_flags, b.kf_flags, kLmPerLink, lm_fill::kf_flags);
}
// `parts` says which of the two are visited
enum { kLmGraph = 1, kLmView = 2 };
template <class A, class B, class Fn>
inline void lm_each(A &a, B &b, int parts, Fn &&fn)
{
    if (parts & kLmGraph) lm_each_graph(a, b, fn);
    if (parts & kLmView) lm_each_view(a, b, fn);
}

// the arrays as 256-byte aligned regions of one block, in the list's order; with `row_set` >= 0 only those of that row set
template <int N>
inline void lm_layout(Regions<N> &R, LmArrays<LmPtr> &P, const LmCounts &c, int parts, int row_set = -1)
{
    lm_each(P, P, parts, [&](auto &p, auto &, LmLen l, auto) {
        if (row_set < 0 || lm_row_set(l) == row_set) R.add(p, lm_len(c, l));
    });
}

// A delta's block: the ascending list of each row set in front of that set's arrays, the graph's part, then the view's.
template <int N>
inline void lm_layout_delta(Regions<N> &R, const int32_t *(&row)[3], LmArrays<LmPtr> &D, const LmCounts &c, int parts)
{
    for (int s = 0; s < 3; ++s) {
        R.add(row[s], lm_rows(c, s));
        lm_layout(R, D, c, kLmGraph, s);
    }
    for (int s = 0; s < 3; ++s) lm_layout(R, D, c, parts & kLmView, s);
}

// copies between instantiations; a zero-length array is not touched and may be NULL
inline void lm_copy(const LmArrays<LmPtr> &dst, const LmArrays<LmPtr> &src, const LmCounts &c, int parts)
{
    lm_each(dst, src, parts, [&](auto *d, auto *s, LmLen l, auto) {
        if (const size_t n = lm_len(c, l)) memcpy(const_cast<void *>((const void *)d), s, n * sizeof(*s));
    });
}
inline void lm_take(LmArrays<LmVec> &dst, const LmArrays<LmPtr> &src, const LmCounts &c, int parts)
{
    lm_each(dst, src, parts, [&](auto &v, auto *s, LmLen l, auto) {
        if (const size_t n = lm_len(c, l)) v.assign(s, s + n);
        else v.clear();
    });
}
// the vectors' own storage
inline LmArrays<LmPtr> lm_data(const LmArrays<LmVec> &V)
{
    LmArrays<LmPtr> P = {};
    lm_each(P, V, kLmGraph | kLmView, [](auto *&p, const auto &v, LmLen, auto) { p = v.data(); });
    return P;
}
// an array that is NULL with a non-zero length
inline bool lm_null_with_length(const LmArrays<LmPtr> &P, const LmCounts &c, int parts)
{
    bool bad = false;
    lm_each(P, P, parts, [&](auto *p, auto *, LmLen l, auto) { bad = bad || (!p && lm_len(c, l) > 0); });
    return bad;
}

}  // namespace aos2
