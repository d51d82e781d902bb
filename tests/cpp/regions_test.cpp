// aos2::Regions and aos2::HostArena (csrc/regions.h) without a GPU: the offsets of a list of typed regions, what bind() writes into
// the fields, and what the arena stages and where.
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

// ---- aos2::HostArena: the same bump rule with staged inputs and typed registration
struct Table {
    const int32_t *none_first = nullptr;   // count 0, the first region
    const float *f = nullptr;
    const double *skipped = nullptr;       // a null source with a count
    const Rec *rec = nullptr;
    Rec *rec3 = nullptr;                   // at(): element 3 of rec
    uint8_t *scratch = nullptr;
    double *none_last = nullptr;           // count 0, the last region
};

// the arena that stages into its own vector -> the number of fields, the staged bytes and the size
static int host_arena_own(size_t &n_fields, size_t &staged, size_t &total)
{
    aos2::HostArena H;
    Table T;
    const float f[3] = {1.5f, 2.5f, 3.5f};
    Rec rec[5];
    for (int i = 0; i < 5; ++i) {
        rec[i].a = i;
        for (int k = 0; k < 4; ++k) rec[i].b[k] = (float)(10 * i + k);
    }
    const int32_t *no_ints = nullptr;
    const double *no_doubles = nullptr;
    CHECK(H.in(T.none_first, no_ints, 0) == 0 && H.size == 0 && H.host_size == 0);
    CHECK(H.in(T.f, f, 3) == 0 && H.size == 12 && H.host_size == 12);
    // a null source takes its room and stages nothing: host_size stays, and what is staged later is still a prefix
    CHECK(H.in(T.skipped, no_doubles, 4) == 256 && H.size == 256 + 32 && H.host_size == 12);
    const size_t o_rec = H.in(T.rec, rec, 5);
    CHECK(o_rec == 512 && sizeof(Rec) == 20 && H.size == 512 + 100 && H.host_size == H.size && H.own.size() == H.host_size);
    CHECK(H.at(T.rec3, o_rec + 3 * sizeof(Rec)) == o_rec + 60 && H.size == 612);   // at() takes no room
    staged = H.host_size;
    CHECK(H.room(T.scratch, 300) == 768 && H.size == 1068 && H.host_size == staged && H.own.size() == staged);
    CHECK(H.room(T.none_last, 0) == 1280 && H.size == 1280 && H.host_size == staged);   // (an empty last region still starts on a boundary)
    CHECK(T.f == nullptr && T.rec3 == nullptr);                                         // registration does not touch a field
    CHECK(memcmp(H.data(), f, sizeof f) == 0 && memcmp(H.data() + o_rec, rec, sizeof rec) == 0);
    n_fields = H.fields.size();
    total = H.size;

    uint8_t *base[2];
    for (int k = 0; k < 2; ++k) {
        base[k] = (uint8_t *)malloc(H.size);
        CHECK(base[k]);
        memcpy(base[k], H.data(), staged);
    }
    for (int k = 0; k < 2; ++k) {   // bind() to one base, then to another: every field follows
        uint8_t *b = base[k];
        H.bind(b);
        CHECK((const uint8_t *)T.none_first == b && (const uint8_t *)T.f == b && (const uint8_t *)T.skipped == b + 256);
        CHECK((const uint8_t *)T.rec == b + 512 && T.rec3 == T.rec + 3 && T.scratch == b + 768 && (uint8_t *)T.none_last == b + 1280);
        CHECK(T.f[2] == 3.5f && T.rec[4].a == 4 && T.rec[4].b[3] == 43.f && T.rec3->a == 3 && T.rec3->b[0] == 30.f);
        T.scratch[299] = (uint8_t)(k + 1);   // the last byte of the last region with bytes lies in the buffer
        CHECK(aos2::span_copy(H.data(), T.f, T.rec3) == H.data() + o_rec + 60);
        CHECK(aos2::bytes_of(T.rec, 5) == 100);
    }
    CHECK(base[0][1067] == 1 && base[1][1067] == 2);
    free(base[0]);
    free(base[1]);
    return 0;
}

// the arena that stages into the caller's buffer of host_cap bytes: the buffer is exactly that long, so a byte past it stops the program
static int host_arena_fixed()
{
    uint8_t a[256];
    for (int i = 0; i < 256; ++i) a[i] = (uint8_t)i;
    const double d = 2.5;
    for (int k = 0; k < 2; ++k) {   // 0: the last push fills the buffer to its last byte; 1: the buffer is one byte short
        const size_t cap = 256 + sizeof(double) - (size_t)k;
        uint8_t *buf = (uint8_t *)malloc(cap);
        CHECK(buf);
        memset(buf, 0xEE, cap);
        aos2::HostArena H;
        H.host = buf;
        H.host_cap = cap;
        const uint8_t *pa = nullptr;
        const double *pd = nullptr;
        CHECK(H.in(pa, a, 256) == 0 && H.host_size == 256 && memcmp(buf, a, 256) == 0 && H.data() == buf);
        CHECK(H.in(pd, &d, 1) == 256 && H.size == 264 && H.host_size == 264);   // host_size moves either way: the caller compares it
        if (k == 0)
            CHECK(H.host_size == H.host_cap && memcmp(buf + 256, &d, sizeof d) == 0);
        else
            CHECK(H.host_size > H.host_cap && buf[256] == 0xEE && buf[cap - 1] == 0xEE);   // nothing was copied
        size_t off = 0;
        CHECK(H.push_fill<int32_t>(1, off) == nullptr && off == 512 && H.host_size == 516);   // no room: NULL
        CHECK(H.own.empty());
        free(buf);
    }
    // push_fill() that fits returns the place in the buffer
    const size_t cap = 256 + 2 * sizeof(double);
    uint8_t *buf = (uint8_t *)malloc(cap);
    CHECK(buf);
    aos2::HostArena H;
    H.host = buf;
    H.host_cap = cap;
    const uint8_t *pa = nullptr;
    H.in(pa, a, 256);
    size_t off = 0;
    double *w = H.push_fill<double>(2, off);
    CHECK(w == (double *)(buf + 256) && off == 256 && H.host_size == cap);
    w[1] = 1.0;   // the buffer's last element
    free(buf);
    return 0;
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

    size_t n_fields = 0, staged = 0, total = 0;
    if (host_arena_own(n_fields, staged, total) || host_arena_fixed()) return 1;
    printf("regions_test ok: %d regions, %zu bytes; host arena ok: %zu fields, %zu of %zu bytes staged\n", kN, R.bytes(), n_fields, staged, total);
    return 0;
}
