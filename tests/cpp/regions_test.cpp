// aos2::Regions (csrc/regions.h) without a GPU: the offsets of a list of typed regions, and what bind() writes into the fields.
// Built with -fsanitize=address,undefined by tests/test_capi_cpu.py: a region that ran past the buffer or a misaligned field
// store would stop the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "regions.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
            return 1;                                                   \
        }                                                               \
    } while (0)

struct Rec {   // an element that is no power of two wide
    int32_t a;
    float b[4];
};

struct Fields {
    float *f = nullptr;
    uint8_t *bytes = nullptr;
    int32_t *none = nullptr;   // count 0
    double *d = nullptr;
    Rec *rec = nullptr;
    const uint8_t *cbytes = nullptr;
    uint64_t *last_none = nullptr;   // count 0 at the end
};

constexpr int kN = 7;

// the same calls for every list: -> offsets and sizes in order of registration
static void lay_out(aos2::Regions<kN> &R, Fields &F, size_t off[kN], size_t size[kN])
{
    const size_t count[kN] = {3, 257, 0, 5, 7, 1, 0};
    const size_t elem[kN] = {sizeof(float), 1, sizeof(int32_t), sizeof(double), sizeof(Rec), 1, sizeof(uint64_t)};
    off[0] = R.add(F.f, count[0]);
    off[1] = R.add(F.bytes, count[1]);
    off[2] = R.add(F.none, count[2]);
    off[3] = R.add(F.d, count[3]);
    off[4] = R.add(F.rec, count[4]);
    off[5] = R.add(F.cbytes, count[5]);
    off[6] = R.add(F.last_none, count[6]);
    for (int i = 0; i < kN; ++i) size[i] = elem[i] * count[i];
}

int main()
{
    CHECK(aos2::up256(0) == 0 && aos2::up256(1) == 256 && aos2::up256(256) == 256 && aos2::up256(257) == 512);
    aos2::Regions<kN> R;
    CHECK(R.bytes() == 0);
    Fields F;
    size_t off[kN], size[kN];
    lay_out(R, F, off, size);
    for (int i = 0; i < kN; ++i) CHECK(off[i] % 256 == 0);
    CHECK(off[0] == 0);
    for (int i = 1; i < kN; ++i) CHECK(off[i] >= off[i - 1] + size[i - 1]);   // disjoint, in order of registration
    CHECK(R.bytes() == off[kN - 1] + size[kN - 1]);
    CHECK(size[kN - 1] == 0 && R.bytes() % 256 == 0);                         // (an empty last region still starts on a boundary)
    CHECK(F.f == nullptr && F.rec == nullptr);                                // add() does not touch a field

    uint8_t *base = (uint8_t *)malloc(R.bytes() ? R.bytes() : 1);
    CHECK(base);
    R.bind(base);
    const void *field[kN] = {F.f, F.bytes, F.none, F.d, F.rec, F.cbytes, F.last_none};
    for (int i = 0; i < kN; ++i) {
        CHECK(field[i] == base + off[i]);
        if (size[i]) base[off[i] + size[i] - 1] = (uint8_t)(i + 1);   // the last byte of every region lies in the buffer
    }
    // ... and through the fields' own types
    F.f[2] = 1.5f;
    F.bytes[256] = 7;
    F.d[4] = 2.5;
    F.rec[6].b[3] = 3.5f;
    CHECK(F.cbytes[0] == 6);
    CHECK(base[off[1] + 256] == 7);

    // a second list with the same calls lays the buffer out the same way; bound elsewhere, the first list's fields stay
    aos2::Regions<kN> R2;
    Fields F2;
    size_t off2[kN], size2[kN];
    lay_out(R2, F2, off2, size2);
    CHECK(memcmp(off, off2, sizeof off) == 0 && R2.bytes() == R.bytes());
    uint8_t *base2 = (uint8_t *)malloc(R2.bytes());
    CHECK(base2);
    R2.bind(base2);
    CHECK((uint8_t *)F2.d == base2 + off[3] && (uint8_t *)F.d == base + off[3]);
    free(base2);
    free(base);
    printf("regions_test ok: %d regions, %zu bytes\n", kN, R.bytes());
    return 0;
}
