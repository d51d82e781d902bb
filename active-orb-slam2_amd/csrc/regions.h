// One buffer laid out as 256-byte aligned regions: the bump rule, and a list that remembers which pointer field is to point
// at which region.  Host only (no HIP): the buffer may be device memory, the list only computes addresses.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace aos2 {

// bump allocation in a buffer of 256-byte aligned pieces: the offset of the next `bytes`, `size` grows past them
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t carve(size_t &size, size_t bytes)
{
    const size_t off = up256(size);
    size = off + bytes;
    return off;
}

// Up to N typed regions of one buffer.  add() fixes a region's offset and registers the field by address (it must stay where
// it is until bind()); bind() points every field at its region once the buffer's base is known.  The list lives in the
// object: nothing here allocates, so it may stand on a per-frame call path.
template <int N>
struct Regions {
    struct Region {
        void *field;   // a T *, of add()'s T
        size_t off;
    };
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
    void bind(uint8_t *base) const
    {
        for (int i = 0; i < n; ++i) {
            const uint8_t *p = base + region[i].off;
            memcpy(region[i].field, &p, sizeof p);   // (every object pointer has this representation; the field's own type is T *)
        }
    }
};

}  // namespace aos2
