// One buffer laid out as 256-byte aligned regions: the bump rule, and the lists that remember which pointer field is to point
// at which region.  Host only (no HIP): the buffer may be device memory, the lists only compute addresses.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

namespace aos2 {

// bump allocation in a buffer of 256-byte aligned pieces: the offset of the next `bytes`, `size` grows past them
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t carve(size_t &size, size_t bytes)
{
    const size_t off = up256(size);
    size = off + bytes;
    return off;
}

// a pointer field, registered by address (it must stay where it is until it is bound), and the offset it will point at
struct Region {
    void *field;   // a T *, of the registering call's T
    size_t off;
};
inline void bind_regions(const Region *region, size_t n, uint8_t *base)
{
    for (size_t i = 0; i < n; ++i) {
        const uint8_t *p = base + region[i].off;
        memcpy(region[i].field, &p, sizeof p);   // (every object pointer has this representation; the field's own type is T *)
    }
}

// Up to N typed regions of one buffer.  add() fixes a region's offset and registers the field; bind() points every field at its
// region once the buffer's base is known.  The list lives in the object: nothing here allocates, so it may stand on a per-frame
// call path.
template <int N>
struct Regions {
    Region region[N];
    int n = 0;
    size_t size = 0;

    // `count` elements of the field's own type at the next 256-byte boundary; returns their offset
    template <class T>
    size_t add(T *&field, size_t count)
    {
        if (n == N) {
            fprintf(stderr, "aos2 regions: more than the list's %d regions\n", N);
            abort();
        }
        const size_t off = carve(size, sizeof(T) * count);
        region[n++] = Region{(void *)&field, off};
        return off;
    }
    size_t bytes() const { return size; }
    void bind(uint8_t *base) const { bind_regions(region, (size_t)n, base); }
};

// One call's arena with its staged inputs: a prefix of the device arena assembled in host memory (the caller's page-locked
// buffer `host`, or `own`), device-only regions after it, and a growable list of the fields that point into either.  Inputs
// are registered before any scratch, so what is staged stays a prefix of host_size bytes.  Not copyable, and so is a layout that
// holds one beside the fields it registered: a copy's list would still name the original's fields.
struct HostArena {
    HostArena() = default;
    HostArena(const HostArena &) = delete;
    HostArena &operator=(const HostArena &) = delete;
    uint8_t *host = nullptr;
    size_t host_cap = 0, host_size = 0;
    std::vector<uint8_t> own;
    size_t size = 0;            // total arena size including device-only scratch
    std::vector<Region> fields;
    const uint8_t *data() const { return host ? host : own.data(); }
    // a null `src` stages nothing; with `host`, a push beyond host_cap copies nothing (the caller compares host_size)
    size_t push(const void *src, size_t bytes)
    {
        const size_t off = carve(size, bytes);
        if (src && bytes) {
            if (!host) {
                own.resize(size);
                memcpy(own.data() + off, src, bytes);
            } else if (size <= host_cap)
                memcpy(host + off, src, bytes);
            host_size = size;
        }
        return off;
    }
    // input produced in place (conversions): returns where to write it
    template <class T>
    T *push_fill(size_t count, size_t &off)
    {
        off = carve(size, count * sizeof(T));
        host_size = size;
        return size <= host_cap ? reinterpret_cast<T *>(host + off) : nullptr;
    }
    // `field` will point at byte `off` of the arena: a second field into an array already placed (ctl + i)
    template <class F>
    size_t at(F *&field, size_t off)
    {
        fields.push_back(Region{(void *)&field, off});
        return off;
    }
    // staged: `count` elements of the host array `src`, of the field's element type
    template <class F, class T>
    size_t in(F *&field, const T *src, size_t count)
    {
        static_assert(std::is_same<std::remove_const_t<F>, T>::value, "the field and the host array differ in type");
        return at(field, push(src, sizeof(F) * count));
    }
    template <class F, class T>
    size_t in(F *&field, const std::vector<T> &src) { return in(field, src.data(), src.size()); }
    // not staged: room for `count` elements of the field's type
    template <class F>
    size_t room(F *&field, size_t count) { return at(field, push(nullptr, sizeof(F) * count)); }
    void bind(uint8_t *base) const { bind_regions(fields.data(), fields.size(), base); }
};

// the bytes of `count` elements of what `field` points at: the size of a copy or a fill through a bound field
template <class T>
inline size_t bytes_of(const T *, size_t count) { return sizeof(T) * count; }

// where a host copy of the arena from `span` on (a field that was bound to the copy's first byte) keeps what `field` points at
template <class S, class T>
inline const uint8_t *span_copy(const uint8_t *copy, const S *span, const T *field)
{
    return copy + ((const uint8_t *)field - (const uint8_t *)span);
}

}  // namespace aos2
