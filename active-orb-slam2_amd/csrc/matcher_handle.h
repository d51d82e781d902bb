// The matcher handle (aos2_matcher_t of include/aos2.h) and the arena every call on it lays its memory out in.  Host only.
// csrc/matcher.hip owns the handle (create / destroy, matcher_init); the geometric solvers that run on it (sim3_ransac.hip,
// pnp_ransac.hip, initializer_ransac.hip) and triangulate.hip are translation units of their own and need no more of the
// matcher than this.  (The matcher's DEVICE layer is search_device.h; no unit that includes this header alone sees it.)
#pragma once
#include <algorithm>
#include <type_traits>
#include <vector>

#include "aos2_common.h"
#include "regions.h"

struct ArenaBind { void *field; size_t tok; };                         // a pointer field and the region offset it will point at
struct ArenaFetch { void *dst; const uint8_t *src; size_t bytes; };    // a result on its way to the caller's array

struct aos2_matcher {
    float nnratio;
    int check_ori;
    int device;
    bool dev_ready = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {};
    aos2::DevBuf<uint8_t> arena;     // one call's inputs | scratch | results (struct Arena)
    aos2::PinnedBuf<uint8_t> h_in;   // page-locked: the inputs on their way up
    aos2::PinnedBuf<uint8_t> h_out;  // page-locked: the results on their way back
    std::vector<ArenaBind> binds;      // Arena: the pointer fields the call in progress has registered, and its pending
    std::vector<ArenaFetch> fetches;   // results (kept by the handle like h_in / h_out: no allocation after the first calls)
    aos2::DevBuf<uint32_t> part;     // hamming partials
    aos2::DevBuf<uint64_t> pool;     // candidate entries of the projection searches (8 B each)
    aos2::DevBuf<float> fr_angle;    // aos2_matcher_search_by_bow_frames: dense key angles of the two frame batches
    aos2::PinnedBuf<uint8_t> fr_host;   // ... and the host copies of their FeatureVectors and counts
    float last_ms = 0;         // device time of the kernels of the last search call
    bool serial_resolve = false;   // AOS2_SERIAL_RESOLVE=1: the one-wave sequential stage B (tests compare both)
};

namespace aos2 {

// binds the handle's device and, on the first call, creates its stream and events (csrc/matcher.hip)
int matcher_init(aos2_matcher *m);

// One call's memory: three regions of the handle's device arena.
//   inputs  (in / hole): assembled in the handle's page-locked host buffer and uploaded with ONE asynchronous
//           copy; the buffer persists between calls, so after the first calls nothing is allocated;
//   scratch (scratch): device only, zeroed by a device memset (never travels);
//   results (out): device only, zeroed; fetch() + finish() bring ALL results back with one copy into a
//           page-locked bounce buffer and scatter them to the caller's arrays.
// (Earlier the whole arena, scratch included, was staged in a pageable vector and uploaded, and every result array
// was a pageable copy of its own: 6.9 ms of host time around 0.06 ms of kernels for 64 SearchByBoW pairs.)
// Where a region starts is known only once every array of the call is staged, and the device arena may move when it
// grows.  So the call that stages an array also names the device-pointer field (of a *Dev struct, or a local) that is
// to point at it, and alloc() -- directly or through upload() -- fills all those fields.  The fields are registered by
// address: they must stay where they are until then (size a vector of per-item structs before its loop), and they
// hold nothing before.  Staging after alloc() aborts (late()).
struct Arena {
    aos2_matcher *m;
    static constexpr size_t kScr = (size_t)1 << 62, kOut = (size_t)1 << 61, kMask = kOut - 1;   // region of an offset: its top bits
    size_t in_size = 0, scr_size = 0, out_size = 0;
    bool frozen = false;
    int err = AOS2_OK;
    explicit Arena(aos2_matcher *m_) : m(m_)
    {
        m->binds.clear();
        m->fetches.clear();
    }
    void late() const
    {
        if (!frozen) return;
        fprintf(stderr, "aos2 matcher arena: an array staged after the layout was fixed\n");
        abort();
    }
    size_t push(const void *src, size_t bytes)
    {
        late();
        const size_t old = in_size, off = carve(in_size, bytes);
        if (in_size > m->h_in.n) {   // grow the page-locked buffer (kept by the handle), contents preserved
            PinnedBuf<uint8_t> nb;
            const int st = nb.alloc(std::max(in_size * 2, (size_t)1 << 20));
            if (st) {
                err = st;
                in_size = old;
                return 0;
            }
            if (old) memcpy(nb.p, m->h_in.p, old);
            m->h_in.release();
            m->h_in = nb;
        }
        if (off > old) memset(m->h_in.p + old, 0, off - old);
        if (bytes) {
            if (src) memcpy(m->h_in.p + off, src, bytes);
            else memset(m->h_in.p + off, 0, bytes);
        }
        return off;
    }
    // `field` will point at `tok`, the region offset that in() / hole() / scratch() / out() returned for an array
    // (plus a few bytes: a second field into that array)
    template <class F>
    size_t bind(F *&field, size_t tok)
    {
        late();
        m->binds.push_back(ArenaBind{&field, tok});
        return tok;
    }
    // input: `bytes` of the host array `src`, of the field's element type
    template <class F, class T>
    size_t in(F *&field, const T *src, size_t bytes)
    {
        static_assert(std::is_same<std::remove_const_t<F>, T>::value, "the field and the host array differ in type");
        return bind(field, push(src, bytes));
    }
    // input the host writes later, through fill_hole(): zero until then
    template <class F>
    size_t hole(F *&field, size_t bytes) { return bind(field, push(nullptr, bytes)); }
    template <class F>
    size_t scratch(F *&field, size_t bytes) { return bind(field, kScr | carve(scr_size, bytes)); }
    template <class F>
    size_t out(F *&field, size_t bytes) { return bind(field, kOut | carve(out_size, bytes)); }
    size_t scr_base() const { return up256(in_size); }
    size_t out_base() const { return scr_base() + up256(scr_size); }
    size_t total() const { return out_base() + up256(out_size); }
    // fixes the layout, sizes the device arena and points every registered field at its array
    int alloc()
    {
        frozen = true;
        if (err) return err;
        if (int st = m->arena.alloc(total() + 256)) return st;
        for (const ArenaBind &b : m->binds) {
            const size_t base = (b.tok & kScr) ? scr_base() : (b.tok & kOut) ? out_base() : 0;
            const uint8_t *p = m->arena.p + base + (b.tok & kMask);
            memcpy(b.field, &p, sizeof p);   // (every object pointer has this representation; the field's own type is F *)
        }
        m->binds.clear();
        return AOS2_OK;
    }
    // after alloc(): the host's bytes for a hole (structs that hold bound device pointers)
    void fill_hole(const void *d_hole, const void *src, size_t bytes)
    {
        memcpy(m->h_in.p + (static_cast<const uint8_t *>(d_hole) - m->arena.p), src, bytes);
    }
    int upload()
    {
        int st = alloc();
        if (st) return st;
        if (in_size) AOS2_HIP_CHECK(hipMemcpyAsync(m->arena.p, m->h_in.p, in_size, hipMemcpyHostToDevice, m->stream));
        if (total() > scr_base()) AOS2_HIP_CHECK(hipMemsetAsync(m->arena.p + scr_base(), 0, total() - scr_base(), m->stream));
        return AOS2_OK;
    }
    // the device array `d_src` (a bound field; normally a result, so that all of them are neighbours) -> dst, delivered by finish()
    void fetch(void *dst, const void *d_src, size_t bytes)
    {
        if (bytes) m->fetches.push_back(ArenaFetch{dst, static_cast<const uint8_t *>(d_src), bytes});
    }
    // one device-to-host copy of the span the results occupy (they are neighbours in the arena; if they are not, one
    // copy each) into the page-locked bounce buffer, a wait for the stream, then the scatter to the caller's arrays
    int finish()
    {
        std::vector<ArenaFetch> &fetches = m->fetches;
        const uint8_t *lo = nullptr, *hi = nullptr;
        size_t sum = 0;
        for (const ArenaFetch &f : fetches) {
            if (!lo || f.src < lo) lo = f.src;
            if (!hi || f.src + f.bytes > hi) hi = f.src + f.bytes;
            sum += (f.bytes + 15) & ~(size_t)15;
        }
        const size_t span = (size_t)(hi - lo);
        const bool one = span <= 4 * sum + 65536;
        int st = m->h_out.alloc((one ? span : sum) + 64);
        if (st) return st;
        if (one) {
            if (span) AOS2_HIP_CHECK(hipMemcpyAsync(m->h_out.p, lo, span, hipMemcpyDeviceToHost, m->stream));
        } else {
            size_t o = 0;
            for (const ArenaFetch &f : fetches) {
                AOS2_HIP_CHECK(hipMemcpyAsync(m->h_out.p + o, f.src, f.bytes, hipMemcpyDeviceToHost, m->stream));
                o += (f.bytes + 15) & ~(size_t)15;
            }
        }
        AOS2_HIP_CHECK(hipStreamSynchronize(m->stream));
        AOS2_HIP_CHECK(hipGetLastError());
        size_t o = 0;
        for (const ArenaFetch &f : fetches) {
            memcpy(f.dst, one ? m->h_out.p + (f.src - lo) : m->h_out.p + o, f.bytes);
            o += (f.bytes + 15) & ~(size_t)15;
        }
        fetches.clear();
        return AOS2_OK;
    }
    // the timed bracket of a call: begin() | the call's kernels | end() = finish() + their device time in last_ms
    int begin()
    {
        AOS2_HIP_CHECK(hipEventRecord(m->ev[0], m->stream));
        return AOS2_OK;
    }
    int end()
    {
        AOS2_HIP_CHECK(hipEventRecord(m->ev[1], m->stream));
        if (int st = finish()) return st;
        (void)hipEventElapsedTime(&m->last_ms, m->ev[0], m->ev[1]);
        return AOS2_OK;
    }
};

}  // namespace aos2
