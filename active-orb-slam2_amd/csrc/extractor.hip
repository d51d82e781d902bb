// Host side of the ORB extractor: plan construction (level sizes, grid cells, resize tables),
// device buffers, stage orchestration on one HIP stream, and the C ABI of include/aos2.h.
// Reference: src/ORBextractor.cc (ctor :410-470, operator() :1043-1105, ComputePyramid :1107-1132,
// ComputeKeyPointsOctTree :765-853).
#include <chrono>
#include <cmath>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "aos2_common.h"
#include "extractor_kernels.h"
#include "octree.h"
#include "stereo.h"

namespace aos2 {

static thread_local std::string g_err;
void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

#define AOS2_FAIL(code, ...) (aos2::set_error(__VA_ARGS__), (code))   // the status to return, with its message

int bind_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device available (%s); this library has no CPU fallback",
                  e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        return AOS2_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) {
        set_error("HIP device %d out of range (0..%d)", device, n - 1);
        return AOS2_ERR_NO_DEVICE;
    }
    AOS2_HIP_CHECK(hipSetDevice(device));
    return AOS2_OK;
}

static const int8_t k_pattern[1024] = {
#include "orb_pattern.inc"
};

constexpr int kEdge = 19;       // EDGE_THRESHOLD src/ORBextractor.cc:74
constexpr int kPatch = 31;      // PATCH_SIZE :72
constexpr int kHalfPatch = 15;  // HALF_PATCH_SIZE :73
constexpr int kMaxLevels = 16;
constexpr int kMaxStreams = 8;

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// ORBextractor's constructor arguments and the host tables derived from them (build_host_tables)
struct Params {
    int nfeatures, nlevels, iniTh, minTh, device;
    float scaleFactor;
    float mvScaleFactor[kMaxLevels], mvInvScaleFactor[kMaxLevels], mvLevelSigma2[kMaxLevels], mvInvLevelSigma2[kMaxLevels];
    int mnFeaturesPerLevel[kMaxLevels], umax[16], gauss7[7];
    unsigned long long umax_nibbles;
    int cap_level, max_kp;   // keypoint_bounds() of the committed plan's image size (of 0 x 0 before the first plan)
};

// The AOS2_* environment switches, read once when the handle is created (read_tuning)
struct Tuning {
    int fast_list = 768;           // AOS2_FAST_LIST: bound of the FAST survivor list (tests force the instalment path with a small value)
    bool pyr_levels = false;       // AOS2_PYRAMID=levels: one launch per pyramid level whatever the batch
    int oct_lds = 0;               // AOS2_OCT_LDS: LDS bytes per octree job (0 = global-scratch path only)
    OctImageLayout oct_pair = {};  // AOS2_OCT_PAIR: total > 0 = two levels per workgroup for batches of >= 8 images (extractor_kernels.h)
    int group_levels = -1;         // AOS2_OCT_GROUP_LEVELS (set: no pair kernel either): levels whose jobs keep helper waves (-1: automatic)
    int chunks = 0;                // AOS2_CHUNKS / aos2_extractor_set_chunks: streams a batch is cut over (0 = automatic)
};

// Everything that depends on the image size: make_plan() fills the host part without a device, upload_plan() the device copies.
struct Plan {
    int w = 0, h = 0;
    std::vector<LevelDev> levels;
    std::vector<CellDev> cells;
    std::vector<int> level_cell_begin, xofs, xab, yofs, yab;
    std::vector<int4> tile_x, tile_y;   // one-launch pyramid (PyrTiles)
    size_t pyr_bytes = 0;               // one image's pyramid block
    size_t oct_cand_total = 0, oct_node_total = 0, slot_total = 0;   // octree scratch, candidate slots per image
    int max_cw = 0, max_ch = 0;
    FastTile fast = {};
    bool pyr_fused = false;
    DevBuf<uint8_t> d_tables[9];   // the device copies (upload_plan) and the typed pointers to them
    const LevelDev *d_levels = nullptr;
    const CellDev *d_cells = nullptr;
    const int *d_level_cell_begin = nullptr;
    ResizeTables tab = {};
    PyrTiles tiles = {};        // (the numbers by make_plan, the two pointers by upload_plan)
    void release() { for (auto &t : d_tables) t.release(); }
};

// The handle's streams and what orders them against the caller's (aos2_extractor_wait_for_stream, aos2_extractor_stream_wait)
struct Streams {
    bool ready = false;
    hipStream_t q[kMaxStreams] = {};         // chunk c of every batch runs on q[c]
    hipEvent_t order_ev[kMaxStreams] = {};   // aos2_extractor_stream_wait
    hipEvent_t input_ev = nullptr, input_fan_ev = nullptr;   // aos2_extractor_wait_for_stream
    int input_waited = 0;   // streams that wait for the inputs announced since the last batch (0 = none announced)
    int last_chunks = 1;    // chunk streams of the last batch
    int used = 0;           // streams the batches since the last wait ran on (<= chunks)
};

struct BatchArgs {   // one batch as the device entry points take it ...
    const uint8_t *d_imgs;
    int batch, w, h, stride;
    size_t image_stride;
    aos2_keypoint_t *d_kps;
    uint8_t *d_desc;
    int cap;
    int32_t *d_nout;
    // ... and, for the host-pointer call (else h_imgs == nullptr), the caller's buffers: each chunk uploads its images in front of its
    // kernels and downloads its results behind them, on its own stream, so the copies of one chunk overlap the kernels of the others
    const uint8_t *h_imgs;
    int h_stride;
    size_t h_image_stride;
    aos2_keypoint_t *h_kps;
    uint8_t *h_desc;
};

// asynchronous batches (aos2_extractor_extract_batch_device_async): enqueued, not yet waited for
struct Flight {
    int in_flight = 0;
    BatchArgs last = {};             // the last enqueued batch: level 0 of the pyramids = its (device) images, its capacity, its d_n_out
    DevBuf<int32_t> d_status;        // sticky [lowest octree failure code, largest n_out] of the batches in flight
    PinnedBuf<int32_t> h_status;
    void release() { d_status.release(); h_status.release(); }
};

// ComputeStereoMatches reads BOTH extractors' pyramid blocks on the left one's first stream: each extractor keeps an event behind
// those kernels, and its next batch waits for it on every chunk stream before it rewrites the pyramids (stereo_guard_wait).
struct StereoGuard {
    hipEvent_t ev = nullptr;
    bool armed = false, captured = false;   // captured: recorded while its stream was being captured (aos2_capture_begin)
    hipStream_t stream = nullptr;           // ... on this stream (the LEFT extractor's)
    aos2_extractor *peer = nullptr;         // the other eye of the last ComputeStereoMatches; always points back (stereo_unpair)
};

// Per-image scratch of a batch: one buffer of [batch][elements per image] per region.  scratch_regions() is the one list of the
// regions (and the order of mem[]); ScratchAt = one image's slices, as the launchers take them.
struct Scratch {
    DevBuf<uint8_t> mem[15];
    int batch_cap = 0;                      // images the buffers hold
    PinnedBuf<int32_t> h_sel_cnt, h_nout;   // host mirrors of the last batch's counts
    void release() { for (auto &m : mem) m.release(); h_sel_cnt.release(); h_nout.release(); batch_cap = 0; }
};
struct ScratchAt {
    ImagePlanes planes;
    uint32_t *slots, *dense;
    int32_t *cell_cnt;
    SelLists sel;
    OctDevScratch oct;
    OctGather gather;
};

struct HostCall {   // device buffers of the host-pointer call (aos2_extractor_extract_batch)
    DevBuf<uint8_t> d_in, d_desc;
    DevBuf<aos2_keypoint_t> d_kps;
    DevBuf<int32_t> d_nout;
    int out_cap = 0;
    void release() { d_in.release(); d_desc.release(); d_kps.release(); d_nout.release(); }
};

struct StereoScratch {   // ComputeStereoMatches (this handle = the left eye)
    DevBuf<int32_t> sad, rows;
    DevBuf<uint8_t> io;
    PinnedBuf<uint8_t> host;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    float ms = 0;
    void release() { sad.release(); rows.release(); io.release(); host.release(); }
};

struct Timing {
    hipEvent_t ev[8] = {};
    float ms[8] = {};   // aos2_extractor_last_timing
    std::chrono::steady_clock::time_point t_enqueue;
};

}  // namespace aos2

using namespace aos2;

struct aos2_extractor {
    Params par = {};
    Tuning tun;
    Streams str;
    Flight flight;
    StereoGuard guard;
    Plan plan;
    Scratch scratch;
    HostCall host;
    StereoScratch stereo;
    Timing tim;
};

namespace aos2 {

static int cv_round_f(float v) { return (int)lrintf(v); }
static int bad_arg(const char *what = "bad argument") { return AOS2_FAIL(AOS2_ERR_ARG, "%s", what); }

// Upper bound of DistributeOctTree's output per level for a w x h image (:539-763): the loop stops at >= N leaves with at
// most 3 extra from the last divide, EXCEPT that its first pass divides all nIni = round(W / H) root nodes unconditionally
// (:549-590), which alone can leave 4 * nIni leaves -- more than N + 3 for wide images with few features
// (found by tools/gpu_fuzz_extractor.py: 838 x 118, nfeatures 100 -> 123 keypoints).
static void keypoint_bounds(const Params &e, int w, int h, int *cap_level, int *max_kp)
{
    int cl = 0, tot = 0;
    for (int l = 0; l < e.nlevels; ++l) {
        int b = e.mnFeaturesPerLevel[l] + 3;
        if (w > 0 && h > 0) {
            const float s = e.mvInvScaleFactor[l];
            const int lw = (int)lrintf((float)w * s), lh = (int)lrintf((float)h * s);
            if (lh - 32 > 0 && lw - 32 > 0) {
                const int nIni = (int)roundf((float)(lw - 32) / (float)(lh - 32));   // round(): half away from zero (:545)
                b = std::max(b, 4 * nIni);
            }
        }
        cl = std::max(cl, b + 1);
        tot += b;
    }
    *cap_level = cl;
    *max_kp = tot;
}

static void build_host_tables(Params *e)
{
    // scale tables :415-432
    e->mvScaleFactor[0] = 1.0f;
    e->mvLevelSigma2[0] = 1.0f;
    for (int i = 1; i < e->nlevels; i++) {
        e->mvScaleFactor[i] = e->mvScaleFactor[i - 1] * e->scaleFactor;
        e->mvLevelSigma2[i] = e->mvScaleFactor[i] * e->mvScaleFactor[i];
    }
    for (int i = 0; i < e->nlevels; i++) {
        e->mvInvScaleFactor[i] = 1.0f / e->mvScaleFactor[i];
        e->mvInvLevelSigma2[i] = 1.0f / e->mvLevelSigma2[i];
    }
    // per-level quotas :436-448
    const float factor = 1.0f / e->scaleFactor;
    float nDesired = e->nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)e->nlevels));
    int sum = 0;
    for (int level = 0; level < e->nlevels - 1; level++) {
        e->mnFeaturesPerLevel[level] = cv_round_f(nDesired);
        sum += e->mnFeaturesPerLevel[level];
        nDesired *= factor;
    }
    e->mnFeaturesPerLevel[e->nlevels - 1] = std::max(e->nfeatures - sum, 0);
    // circular patch extents :454-470
    const int vmax = (int)std::floor(kHalfPatch * std::sqrt(2.f) / 2 + 1);
    const int vmin = (int)std::ceil(kHalfPatch * std::sqrt(2.f) / 2);
    const double hp2 = kHalfPatch * kHalfPatch;
    for (int v = 0; v <= vmax; ++v) e->umax[v] = (int)lrint(std::sqrt(hp2 - v * v));
    for (int v = kHalfPatch, v0 = 0; v >= vmin; --v) {
        while (e->umax[v0] == e->umax[v0 + 1]) ++v0;
        e->umax[v] = v0;
        ++v0;
    }
    // cv::getGaussianKernel(7, 2, CV_32F) -> 8 fractional bits (createSeparableLinearFilter 8U path)
    float cf[7];
    double s = 0;
    for (int i = 0; i < 7; ++i) {
        const double x = i - 3.0;
        cf[i] = (float)std::exp(-0.5 / 4.0 * x * x);
        s += cf[i];
    }
    s = 1. / s;
    for (int i = 0; i < 7; ++i) {
        cf[i] = (float)(cf[i] * s);
        e->gauss7[i] = (int)lrint((double)cf[i] * 256.0);
    }
    keypoint_bounds(*e, 0, 0, &e->cap_level, &e->max_kp);   // for a "normal" aspect ratio; ensure_plan() raises them for the actual image size
    e->umax_nibbles = 0;
    for (int v = 0; v < 16; ++v) e->umax_nibbles |= (unsigned long long)(e->umax[v] & 15) << (4 * v);
}

static short sat_short(float v)
{
    int i = (int)lrintf(v);
    return (short)std::min(32767, std::max(-32768, i));
}

// cv::resize() coefficient tables for src -> dst (INTER_LINEAR, 8U fixed point)
static void resize_tables(int sw, int sh, int dw, int dh, std::vector<int> &xofs, std::vector<int> &xab,
                          std::vector<int> &yofs, std::vector<int> &yab)
{
    const double inv_sx = (double)dw / sw, inv_sy = (double)dh / sh;
    const double scale_x = 1. / inv_sx, scale_y = 1. / inv_sy;
    for (int dx = 0; dx < dw; ++dx) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)std::floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        const short a0 = sat_short((1.f - fx) * 2048), a1 = sat_short(fx * 2048);
        xofs.push_back(sx);
        xab.push_back((int)((uint32_t)(uint16_t)a0 | ((uint32_t)(uint16_t)a1 << 16)));
    }
    for (int dy = 0; dy < dh; ++dy) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)std::floor(fy);
        fy -= sy;
        const short b0 = sat_short((1.f - fy) * 2048), b1 = sat_short(fy * 2048);
        yofs.push_back(sy);
        yab.push_back((int)((uint32_t)(uint16_t)b0 | ((uint32_t)(uint16_t)b1 << 16)));
    }
    // the kernel reads x tables as int4: pad every level's table to a multiple of 4 entries
    for (std::vector<int> *t : {&xofs, &xab, &yofs, &yab})
        while (t->size() % 4) t->push_back(t->back());
}

// grid cells of level l (:768-806), appended to P.cells; `slot` = the running candidate-slot offset inside one image's block
static int plan_cells(Plan &P, int l, size_t &slot)
{
    const LevelDev &L = P.levels[l];
    const int minBorderX = kEdge - 3, minBorderY = minBorderX;
    const int maxBorderX = L.w - kEdge + 3, maxBorderY = L.h - kEdge + 3;
    const float width = (float)(maxBorderX - minBorderX), height = (float)(maxBorderY - minBorderY);
    const int nCols = (int)(width / 30.f), nRows = (int)(height / 30.f);
    const int wCell = (int)std::ceil(width / nCols), hCell = (int)std::ceil(height / nRows);
    P.level_cell_begin.push_back((int)P.cells.size());
    for (int i = 0; i < nRows; i++) {
        const int iniY = minBorderY + i * hCell;
        int maxY = iniY + hCell + 6;
        if (iniY >= maxBorderY - 3) continue;
        if (maxY > maxBorderY) maxY = maxBorderY;
        for (int j = 0; j < nCols; j++) {
            const int iniX = minBorderX + j * wCell;
            int maxX = iniX + wCell + 6;
            if (iniX >= maxBorderX - 6) continue;
            if (maxX > maxBorderX) maxX = maxBorderX;
            CellDev c{};
            c.level = (int16_t)l;
            c.vx0 = (int16_t)(iniX + 3);
            c.vy0 = (int16_t)(iniY + 3);
            c.cw = (int16_t)(maxX - iniX - 6);
            c.ch = (int16_t)(maxY - iniY - 6);
            if (c.cw <= 0 || c.ch <= 0) continue;  // sub-image < 7 px: cv::FAST evaluates nothing
            if (c.cw > 64) return AOS2_FAIL(AOS2_ERR_ARG, "cell width %d > 64 unsupported", (int)c.cw);
            c.slot_off = (int32_t)slot;
            const uint32_t nq = (uint32_t)(c.cw + 3) / 4;
            c.inv_nq = 65536u / nq + 1;
            c.inv_ndw = 65536u / (nq + 2) + 1;
            c.inv_n16 = 65536u / ((nq + 2 + 3) / 4) + 1;
            if (L.off > 0xffffffffull || L.pitch > 0xffff)
                return AOS2_FAIL(AOS2_ERR_ARG, "pyramid of a %dx%d image exceeds the 32-bit plane offsets", P.w, P.h);
            c.pitch = (uint16_t)L.pitch;
            c.plane_off = (uint32_t)L.off;
            slot += (size_t)((c.cw + 1) / 2) * ((c.ch + 1) / 2);
            P.max_cw = std::max<int>(P.max_cw, c.cw);
            P.max_ch = std::max<int>(P.max_ch, c.ch);
            P.cells.push_back(c);
        }
    }
    return AOS2_OK;
}

// Tiles of the one-launch pyramid.  A workgroup owns [B_k(i), B_k(i + 1)) of level k along each axis, B_k(i) = the level-0
// boundary 64 i divided by the level's scale (any monotone choice works); what it must COMPUTE at level k is that plus the
// sources of what it computes at level k + 1 (read off the resize tables), from the top level down.
static void plan_pyramid_tiles(const Params &par, Plan &P)
{
    const int L = par.nlevels, TS = 64;
    PyrTiles &T = P.tiles;
    T.ntx = (P.w + TS - 1) / TS;
    T.nty = (P.h + TS - 1) / TS;
    int maxw = 0, maxh = 0;
    auto axis = [&](bool is_x, int nt, std::vector<int4> &out, int &maxn) {
        out.assign((size_t)L * nt, int4{0, 0, 0, 0});
        for (int i = 0; i < nt; ++i) {
            int n0 = 0, n1 = 0;   // need of level k + 1
            for (int k = L - 1; k >= 0; --k) {
                const int dim = is_x ? P.levels[k].w : P.levels[k].h;
                auto bound = [&](int j) {
                    if (j >= nt) return dim;
                    return std::min(dim, (int)std::lround((double)(TS * j) / (double)par.mvScaleFactor[k]));
                };
                int o0 = bound(i), o1 = bound(i + 1);
                if (k == 0) o0 = o1 = 0;   // level 0 is the caller's image: nothing to own
                int c0 = o0, c1 = o1;
                if (k + 1 < L && n1 > n0) {   // sources of the region of level k + 1
                    const std::vector<int> &tab = is_x ? P.xofs : P.yofs;
                    const int base = is_x ? P.levels[k + 1].tab_x : P.levels[k + 1].tab_y;
                    const int lo = std::min(std::max(tab[base + n0], 0), dim - 1);
                    const int hi = std::min(std::max(tab[base + n1 - 1] + 1, 0), dim - 1);
                    if (c1 > c0) {
                        c0 = std::min(c0, lo);
                        c1 = std::max(c1, hi + 1);
                    } else {
                        c0 = lo;
                        c1 = hi + 1;
                    }
                }
                out[(size_t)k * nt + i] = int4{o0, o1, c0, c1};
                maxn = std::max(maxn, c1 - c0);
                n0 = c0;
                n1 = c1;
            }
        }
    };
    axis(true, T.ntx, P.tile_x, maxw);
    axis(false, T.nty, P.tile_y, maxh);
    T.buf_pitch = (maxw + 3) & ~3;
    T.buf_rows = maxh;
    T.lds = 2 * (size_t)T.buf_pitch * T.buf_rows + (size_t)(2 * T.buf_pitch + 2 * T.buf_rows) * sizeof(int) + 16;
}

// The host part of the plan for w x h images: arithmetic only -- no HIP call, no environment -- so it runs without a device
// (aos2_debug_extractor_plan).  `P` comes in fresh and is the caller's to discard on an error.
static int make_plan(const Params &par, const Tuning &tun, int w, int h, Plan &P)
{
    // smallest level must admit at least one 30-px cell in both directions (:783-786)
    const float s_top = par.mvInvScaleFactor[par.nlevels - 1];
    if (cv_round_f((float)w * s_top) - 32 < 30 || cv_round_f((float)h * s_top) - 32 < 30)
        return AOS2_FAIL(AOS2_ERR_TOO_SMALL, "image %dx%d too small for %d pyramid levels", w, h, par.nlevels);
    if (w > 4000 || h > 4000) return AOS2_FAIL(AOS2_ERR_ARG, "image %dx%d exceeds the 12-bit candidate packing", w, h);
    P.w = w;
    P.h = h;
    size_t off = 0, slot = 0;
    for (int l = 0; l < par.nlevels; ++l) {
        LevelDev L{};
        const float s = par.mvInvScaleFactor[l];
        L.w = cv_round_f((float)w * s);   // :1112
        L.h = cv_round_f((float)h * s);
        L.pitch = (L.w + 4 + 15) & ~15;   // >= w+4 so 32-bit tile loads may overrun a row end
        L.off = off;
        off += up256((size_t)L.pitch * (L.h + 1));
        L.nfeat = par.mnFeaturesPerLevel[l];
        L.scaled_patch = (int)(kPatch * par.mvScaleFactor[l]);
        L.scale = par.mvScaleFactor[l];
        L.tab_x = (int)P.xofs.size();
        L.tab_y = (int)P.yofs.size();
        if (l > 0)
            resize_tables(P.levels[l - 1].w, P.levels[l - 1].h, L.w, L.h, P.xofs, P.xab, P.yofs, P.yab);
        P.levels.push_back(L);
        if (int st = plan_cells(P, l, slot)) return st;
    }
    P.pyr_bytes = off;
    P.slot_total = (slot + 63) & ~(size_t)63;
    for (int l = 0; l < par.nlevels; ++l) {
        LevelDev &L = P.levels[l];
        size_t cap = 0;
        const int c1 = l + 1 < par.nlevels ? P.level_cell_begin[l + 1] : (int)P.cells.size();
        for (int c = P.level_cell_begin[l]; c < c1; ++c) cap += (size_t)((P.cells[c].cw + 1) / 2) * ((P.cells[c].ch + 1) / 2);
        L.oct_cand_off = (int)P.oct_cand_total;
        L.oct_cand_cap = (int)cap;
        P.oct_cand_total += (cap + 63) & ~(size_t)63;
        L.oct_node_off = (int)P.oct_node_total;
        L.oct_node_cap = oct_max_nodes((int)cap, L.nfeat);
        P.oct_node_total += (size_t)L.oct_node_cap;
    }
    // LDS tile: [4-byte left halo | nq quads | 4-byte right halo] per row, evaluated column 0 at byte 4
    FastTile &F = P.fast;
    F.TP = (4 * ((P.max_cw + 3) / 4) + 8 + 15) & ~15;   // (a multiple of 16: the tile is staged 16 bytes per lane)
    F.TH = P.max_ch + 6;
    F.SP = (P.max_cw + 2 + 3) & ~3;
    // every pixel of every 4-px group may survive the pre-test (columns >= cw of the last group are
    // only dropped in phase 2), so size the list for whole groups
    F.list_cap = (4 * ((P.max_cw + 3) / 4) * P.max_ch + 7) & ~7;
    F.keep_cap = ((P.max_cw + 1) / 2) * ((P.max_ch + 1) / 2);          // NMS survivors are >= 2 px apart
    // The survivor list is bounded (typical cells produce 100-200 survivors); a cell that produces more is
    // scored in instalments.  The smaller LDS footprint doubles the waves per SIMD.
    F.list_cap = std::min(F.list_cap, (tun.fast_list + 7) & ~7);
    F.lds = (((size_t)F.TP * F.TH + 15) & ~(size_t)15) + (((size_t)F.SP * (F.TH - 4) + 15) & ~(size_t)15) +
            (size_t)F.list_cap * 2 + 16;
    plan_pyramid_tiles(par, P);
    // steep pyramids (scale factor towards 2) need hundreds of pixels of halo at level 0: those keep one launch per level
    P.pyr_fused = par.nlevels > 1 && P.tiles.lds <= 60 * 1024 && !tun.pyr_levels;
    return AOS2_OK;
}

// The plan's tables on the device: every (host vector, device pointer) pair is named once, in the list below.
static int upload_plan(Plan &P)
{
    int i = 0, st;
    auto table = [&](const auto &host, auto *&dev) -> int {
        DevBuf<uint8_t> &buf = P.d_tables[i++];
        const size_t bytes = host.size() * sizeof(host[0]);
        if (int st_ = buf.alloc(bytes)) return st_;
        if (bytes) AOS2_HIP_CHECK(hipMemcpy(buf.p, host.data(), bytes, hipMemcpyHostToDevice));
        dev = reinterpret_cast<std::remove_reference_t<decltype(dev)>>(buf.p);
        return AOS2_OK;
    };
    if ((st = table(P.levels, P.d_levels)) || (st = table(P.cells, P.d_cells)) ||
        (st = table(P.level_cell_begin, P.d_level_cell_begin)) || (st = table(P.xofs, P.tab.xofs)) ||
        (st = table(P.xab, P.tab.xab)) || (st = table(P.yofs, P.tab.yofs)) || (st = table(P.yab, P.tab.yab)) ||
        (st = table(P.tile_x, P.tiles.tile_x)) || (st = table(P.tile_y, P.tiles.tile_y)))
        return st;
    return AOS2_OK;
}

// The plan of the handle for w x h images.  A new one is built aside and COMMITTED -- moved into the handle, with the keypoint
// capacities and the scratch sizing that depend on it -- only after its last upload succeeded: a failure leaves the handle
// with the plan it had (or none), never with a half-built one that a later call of the same size would take for complete.
static int ensure_plan(aos2_extractor *e, int w, int h)
{
    if (e->plan.w == w && e->plan.h == h) return AOS2_OK;
    Plan P;
    int st = make_plan(e->par, e->tun, w, h, P);
    if (st == AOS2_OK) st = upload_plan(P);
    if (st) {
        P.release();
        return st;
    }
    e->plan.release();
    e->plan = std::move(P);
    keypoint_bounds(e->par, w, h, &e->par.cap_level, &e->par.max_kp);
    e->scratch.batch_cap = 0;  // the scratch layout depends on the plan
    return AOS2_OK;
}

static int init_device(aos2_extractor *e)
{
    int st = bind_device(e->par.device);
    if (st) return st;
    if (e->str.ready) return AOS2_OK;
    for (auto &q : e->str.q)
        if ((st = stream_create(&q, false))) return st;
    for (auto &ev : e->tim.ev) AOS2_HIP_CHECK(hipEventCreate(&ev));
    if (e->tun.oct_pair.total > 0 && prepare_octree_pair_kernel(e->tun.oct_pair.total) != 0) {
        (void)hipGetLastError();
        e->tun.oct_pair.total = 0;  // the runtime refuses that much LDS: keep the per-job kernel
    }
    int r = upload_constants(k_pattern, e->par.umax, e->par.gauss7, e->str.q[0]);
    if (r != 0) return AOS2_FAIL(AOS2_ERR_HIP, "constant upload failed: %s", hipGetErrorString((hipError_t)r));
    if ((st = e->flight.d_status.alloc(2))) return st;
    if ((st = e->flight.h_status.alloc(2))) return st;
    AOS2_HIP_CHECK(hipMemsetAsync(e->flight.d_status.p, 0, 2 * sizeof(int32_t), e->str.q[0]));
    AOS2_HIP_CHECK(hipStreamSynchronize(e->str.q[0]));
    e->str.ready = true;
    return AOS2_OK;
}

// The region list of the scratch: every per-image array once, as (the field of ScratchAt that points at it, elements per image).
// Points a's fields at image b0's slices; with batch > 0 it first grows every buffer to hold `batch` images.
static int scratch_regions(aos2_extractor *e, int batch, int b0, ScratchAt &a)
{
    const Plan &P = e->plan;
    const size_t L = (size_t)e->par.nlevels, sel = L * e->par.cap_level, cand = P.oct_cand_total, node = P.oct_node_total;
    int i = 0, st = AOS2_OK;
    auto region = [&](auto *&field, size_t per_image, size_t slack = 0) {
        using T = std::remove_reference_t<decltype(*field)>;
        DevBuf<uint8_t> &m = e->scratch.mem[i++];
        if (batch > 0 && st == AOS2_OK) st = m.alloc(sizeof(T) * per_image * batch + slack);
        field = reinterpret_cast<T *>(m.p) + per_image * b0;
    };
    region(a.planes.pyr, P.pyr_bytes, 256);   // (+ 256: 32-bit tile loads may overrun the last plane)
    region(a.slots, P.slot_total);
    region(a.dense, P.slot_total);
    region(a.cell_cnt, P.cells.size());
    region(a.gather.level_cnt, L);
    region(a.sel.sel, sel);
    region(a.sel.sel_cnt, L);
    region(a.oct.xs, cand);
    region(a.oct.ys, cand);
    region(a.oct.sc, cand);
    region(a.oct.perm, cand);
    region(a.oct.tmp, cand);
    region(a.oct.pairs, 4 * node);
    region(a.oct.out_idx, sel);
    region(a.oct.nodes, node);
    return st;
}

// Image b0's slices of the last batch's images and of the scratch, as launch arguments: the only place that slices by image.
static ScratchAt scratch_at(aos2_extractor *e, int b0)
{
    const Plan &P = e->plan;
    const BatchArgs &B = e->flight.last;   // (level 0 is the caller's image, no copy; levels >= 1 live in the pyramid region)
    ScratchAt a;
    scratch_regions(e, 0, b0, a);   // (the three aggregates below keep the pointers this has just put into them)
    a.planes = ImagePlanes{B.d_imgs + (size_t)b0 * B.image_stride, B.image_stride, B.stride, a.planes.pyr, P.pyr_bytes};
    a.sel = SelLists{a.sel.sel, (size_t)e->par.nlevels * e->par.cap_level, e->par.cap_level, a.sel.sel_cnt};
    a.oct.cand_stride = P.oct_cand_total;
    a.oct.node_stride = P.oct_node_total;
    a.gather = OctGather{P.d_cells, P.d_level_cell_begin, a.slots, P.slot_total, a.cell_cnt, (int)P.cells.size(), a.gather.level_cnt};
    return a;
}

// The scratch for (at least) `batch` images of the current plan.
static int ensure_batch(aos2_extractor *e, int batch)
{
    Scratch &S = e->scratch;
    if (batch <= S.batch_cap) return AOS2_OK;
    S.batch_cap = e->flight.last.batch = 0;   // (nothing is in flight here; until this succeeds there is no batch for the taps to read)
    ScratchAt a;
    int st;
    if ((st = scratch_regions(e, batch, 0, a))) return st;
    if ((st = S.h_sel_cnt.alloc((size_t)e->par.nlevels * batch))) return st;
    if ((st = S.h_nout.alloc(batch))) return st;
    // row h of every plane (1 guard row) and pitch padding are read by 32-bit tile loads: keep
    // them defined
    AOS2_HIP_CHECK(hipMemsetAsync(a.planes.pyr, 0, e->plan.pyr_bytes * batch + 256, e->str.q[0]));
    // The chunks of the batch that follows run on streams of their own: they must not start while this memset is still running on
    // the first stream (round 4: a fresh handle given 1920 images -- 2 GB of pyramid, a memset of ~1 ms -- had the pyramids of its
    // second and third chunk zeroed under them; 720 images lost a few frames at the end, 256 none).  Once per capacity growth.
    AOS2_HIP_CHECK(hipStreamSynchronize(e->str.q[0]));
    S.batch_cap = batch;
    return AOS2_OK;
}

// true while `s` records for aos2_capture_begin / _end (csrc/replay.hip)
static bool stream_is_capturing(hipStream_t s)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st == hipStreamCaptureStatusActive;
}

static const char *octree_failure_text(int code)
{
    return code == -4   ? "candidate capacity exceeded"
           : code == -1 ? "level more than twice as tall as wide: round(width / height) == 0, the reference's DistributeOctTree "
                          "divides by zero (src/ORBextractor.cc:545)"
                        : "node arena exhausted";
}

// Waits for every batch in flight; reports the sticky device status of all of them and, in detail, the last one.
static int finish_device(aos2_extractor *e)
{
    Flight &F = e->flight;
    hipStream_t *q = e->str.q;
    if (F.in_flight == 0) return AOS2_OK;
    if (stream_is_capturing(q[0]))   // (refused before the runtime sees the wait: it would invalidate the recording)
        return AOS2_FAIL(AOS2_ERR_ARG, "the extractor's stream is recording (aos2_capture_begin): a host wait -- aos2_extractor_wait, a "
                                       "synchronous call, a change of batch size or geometry -- cannot be recorded");
    const int L = e->par.nlevels, batch = F.last.batch, cap = F.last.cap;
    const int32_t *h_sel_cnt = e->scratch.h_sel_cnt.p, *h_nout = e->scratch.h_nout.p;
    for (int c = 1; c < kMaxStreams; ++c) AOS2_HIP_CHECK(hipStreamSynchronize(q[c]));
    // status words + the counts of the last batch: three small copies behind the last chunk of stream 0, one wait
    AOS2_HIP_CHECK(hipMemcpyAsync(F.h_status.p, F.d_status.p, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, q[0]));
    AOS2_HIP_CHECK(hipMemcpyAsync(e->scratch.h_sel_cnt.p, scratch_at(e, 0).sel.sel_cnt, sizeof(int32_t) * (size_t)L * batch,
                                  hipMemcpyDeviceToHost, q[0]));
    AOS2_HIP_CHECK(hipMemcpyAsync(e->scratch.h_nout.p, F.last.d_nout, sizeof(int32_t) * (size_t)batch, hipMemcpyDeviceToHost, q[0]));
    AOS2_HIP_CHECK(hipStreamSynchronize(q[0]));
    const int32_t status[2] = {F.h_status.p[0], F.h_status.p[1]};
    F.in_flight = 0;
    e->str.used = 0;
    AOS2_HIP_CHECK(hipGetLastError());
    for (int i = 0; i < 5; ++i) (void)hipEventElapsedTime(&e->tim.ms[i], e->tim.ev[i], e->tim.ev[i + 1]);
    e->tim.ms[5] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - e->tim.t_enqueue).count();
    if (status[0] != 0 || status[1] != 0) AOS2_HIP_CHECK(hipMemset(F.d_status.p, 0, sizeof(status)));
    for (int i = 0; i < L * batch; ++i)
        if (h_sel_cnt[i] < 0)
            return AOS2_FAIL(AOS2_ERR_CAPACITY, "octree stage failed for image %d level %d (code %d: %s)", i / L, i % L, h_sel_cnt[i],
                             octree_failure_text(h_sel_cnt[i]));
    for (int b = 0; b < batch; ++b)
        if (h_nout[b] > cap) return AOS2_FAIL(AOS2_ERR_CAPACITY, "image %d has %d keypoints, capacity %d", b, h_nout[b], cap);
    // earlier batches of the same flight (their per-image counts are gone; the sticky words are not)
    if (status[0] < 0)
        return AOS2_FAIL(AOS2_ERR_CAPACITY, "octree stage failed in an earlier batch of this flight (code %d: %s)", status[0],
                         octree_failure_text(status[0]));
    if (status[1] > cap)
        return AOS2_FAIL(AOS2_ERR_CAPACITY, "an earlier batch of this flight produced %d keypoints for one image, capacity %d", status[1], cap);
    return AOS2_OK;
}

// Ends e's pairing with the other eye, in both directions: called before either handle is paired with a third one and before e is
// destroyed, so no handle keeps a pointer to a partner that does not point back.  A guard that names a stream of the other handle
// forgets it: an event of executed work stays valid (the next batch still waits for it); one recorded in a capture is disarmed.
static void stereo_unpair(aos2_extractor *e)
{
    aos2_extractor *p = e->guard.peer;
    if (!p) return;
    e->guard.peer = p->guard.peer = nullptr;
    auto forget = [](StereoGuard &g, const Streams &of) {
        for (hipStream_t q : of.q)
            if (q && g.stream == q) {
                if (g.captured) g.armed = g.captured = false;
                g.stream = nullptr;
            }
    };
    forget(p->guard, e->str);
    forget(e->guard, p->str);
}

// Stereo kernels enqueued since the last batch may still read this extractor's pyramids: the `chunks` streams of the batch
// that is about to rewrite them wait for the guard first.
static int stereo_guard_wait(aos2_extractor *e, int chunks)
{
    StereoGuard &g = e->guard;
    if (!g.armed) return AOS2_OK;
    // An event of a recording (aos2_capture_begin) and one of executed work cannot wait for each other.  Executed batch behind a
    // replayed recording: the guard is recorded again, now, on the stream the recording ran on (behind every launched replay).
    // Recording behind executed work: no wait (a sequence is run, and waited for, before it is recorded: include/aos2.h).
    const bool rec = stream_is_capturing(e->str.q[0]);
    if (!rec && g.captured) {
        AOS2_HIP_CHECK(hipEventRecord(g.ev, g.stream));
        g.captured = false;
    }
    if (rec == g.captured)
        for (int c = 0; c < chunks; ++c) AOS2_HIP_CHECK(hipStreamWaitEvent(e->str.q[c], g.ev, 0));
    g.armed = false;
    return AOS2_OK;
}

// The chunk streams of a batch, ordered behind the inputs announced by aos2_extractor_wait_for_stream.
static int begin_chunks(aos2_extractor *e, int batch, bool host_io, int &chunks)
{
    // The batch is cut into chunks that run on separate streams: the octree kernel is
    // latency-bound (one wave per (image, level), ~0.15 ms whatever the batch size) and leaves
    // the CUs idle, so a chunk's octree overlaps the VALU-bound kernels of the other chunks (and, with the
    // asynchronous call, of the next batch).  Measured at B=256, K steps in flight / synchronous call:
    // 2 chunks 0.933 / 0.964 ms, 3 chunks 0.855 / 0.967, 4 chunks 0.852 / 0.971 (needs GPU_MAX_HW_QUEUES=8: the
    // runtime's default of 4 hardware queues puts two of the 4 streams on one queue, 1.16 ms), 6: 1.08, 8: 1.28
    // (smaller chunks lose to kernel tails and queue sharing; replaying each chunk as one hipGraph changed nothing).
    Streams &S = e->str;
    chunks = e->tun.chunks > 0 ? e->tun.chunks : (batch >= 96 ? 3 : batch >= 64 ? 2 : 1);
    if (host_io && e->tun.chunks <= 0 && batch >= 32) chunks = 4;   // copy / compute pipeline of the host-pointer call
    chunks = std::min(chunks, std::min(batch, kMaxStreams));
    S.used = std::max(S.used, chunks);
    if (S.input_waited > 0 && chunks > S.input_waited) {   // (aos2_extractor_wait_for_stream: stream 0 waits for the inputs already)
        if (!S.input_fan_ev) AOS2_HIP_CHECK(hipEventCreateWithFlags(&S.input_fan_ev, hipEventDisableTiming));
        AOS2_HIP_CHECK(hipEventRecord(S.input_fan_ev, S.q[0]));
        for (int c = S.input_waited; c < chunks; ++c) AOS2_HIP_CHECK(hipStreamWaitEvent(S.q[c], S.input_fan_ev, 0));
    }
    S.input_waited = 0;
    S.last_chunks = chunks;
    return AOS2_OK;
}

// Images [b0, b0 + nb) of the batch on stream s: (upload,) pyramid, FAST, octree, descriptors(, download).
static int enqueue_chunk(aos2_extractor *e, const BatchArgs &B, int b0, int nb, hipStream_t s, bool timed)
{
    const Plan &P = e->plan;
    const int L = e->par.nlevels, NC = (int)P.cells.size(), cap = B.cap;
    const ScratchAt a = scratch_at(e, b0);
    hipEvent_t *ev = e->tim.ev;
    aos2_keypoint_t *d_kps = B.d_kps + (size_t)b0 * cap;
    uint8_t *d_desc = B.d_desc + (size_t)b0 * cap * 32;
    if (B.h_imgs) {
        uint8_t *dst = const_cast<uint8_t *>(a.planes.img0);
        const uint8_t *src = B.h_imgs + (size_t)b0 * B.h_image_stride;
        if (B.h_stride == B.w && B.h_image_stride == (size_t)B.w * B.h)
            AOS2_HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)nb * B.w * B.h, hipMemcpyHostToDevice, s));
        else
            for (int b = 0; b < nb; ++b)
                AOS2_HIP_CHECK(hipMemcpy2DAsync(dst + (size_t)b * B.image_stride, (size_t)B.stride, src + (size_t)b * B.h_image_stride,
                                                (size_t)B.h_stride, (size_t)B.w, (size_t)B.h, hipMemcpyHostToDevice, s));
    }
    if (timed) AOS2_HIP_CHECK(hipEventRecord(ev[0], s));
    // one launch for a few frames (latency: 36 -> ~15 us per frame); the per-level kernel is the throughput form (4 pixels per
    // lane, packed arithmetic: 0.135 ms per 256 frames against 0.38 ms for the fused one, which works pixel by pixel)
    if (P.pyr_fused && nb < 8)
        launch_pyramid_fused(a.planes, P.d_levels, L, P.tiles, P.tab, nb, s);
    else
        for (int l = 1; l < L; ++l) launch_resize(a.planes, P.levels.data(), l, P.tab, nb, s);
    if (timed) AOS2_HIP_CHECK(hipEventRecord(ev[1], s));
    launch_fast(a.planes, P.d_cells, NC, e->par.iniTh, e->par.minTh, P.fast, a.slots, P.slot_total, a.cell_cnt, nb, s);
    if (timed) AOS2_HIP_CHECK(hipEventRecord(ev[2], s));
    // (timing slot [2], once a candidate compaction kernel: every octree job now gathers its own candidates from the cell slots)
    if (timed) AOS2_HIP_CHECK(hipEventRecord(ev[3], s));
    const Tuning &T = e->tun;   // (the pair form from 8 images on; fewer: the helper-wave form of the per-job kernel)
    launch_octree(a.dense, P.slot_total, a.gather, P.d_levels, L, nb, a.oct, a.sel, T.oct_pair.total > 0 && nb >= 8 ? &T.oct_pair : nullptr,
                  T.oct_lds, T.group_levels >= 0 ? T.group_levels : (nb < 8 ? 2 : 0), s);
    if (timed) AOS2_HIP_CHECK(hipEventRecord(ev[4], s));
    launch_describe(a.planes, P.d_levels, L, a.sel, d_kps, d_desc, cap, B.d_nout + b0, nb, e->par.umax_nibbles,
                    e->flight.d_status.p, s);
    if (timed) AOS2_HIP_CHECK(hipEventRecord(ev[5], s));
    if (B.h_imgs) {
        AOS2_HIP_CHECK(hipMemcpyAsync(B.h_kps + (size_t)b0 * cap, d_kps, sizeof(aos2_keypoint_t) * (size_t)nb * cap,
                                      hipMemcpyDeviceToHost, s));
        AOS2_HIP_CHECK(hipMemcpyAsync(B.h_desc + (size_t)b0 * cap * 32, d_desc, (size_t)nb * cap * 32, hipMemcpyDeviceToHost, s));
    }
    // (the per-level and per-image counts of the LAST batch of a flight are fetched once by finish_device(); errors of
    // earlier batches travel in the sticky status words -- no blit kernels between the chunks' launches)
    return AOS2_OK;
}

// the argument check of the device entry points (enqueue_device, run_device)
static int check_device_args(const aos2_extractor *e, const BatchArgs &B)
{
    const bool ok = e && B.d_imgs && B.d_kps && B.d_desc && B.d_nout && B.batch > 0 && B.w > 0 && B.h > 0 && B.stride >= B.w && B.cap > 0;
    return ok ? AOS2_OK : bad_arg();
}

// Enqueues one batch on the handle's streams and returns; finish_device() completes it.  Chunk c of every batch
// uses stream c and the scratch of its own image range, so consecutive batches are ordered per stream and may be
// in flight together: a chunk's latency-bound octree then overlaps the next batch's kernels on the other streams.
static int enqueue_device(aos2_extractor *e, const BatchArgs &B)
{
    int st, chunks = 1;
    if ((st = check_device_args(e, B))) return st;
    e->tim.t_enqueue = std::chrono::steady_clock::now();
    Flight &F = e->flight;
    if ((st = init_device(e))) return st;
    // Batches of one flight share the scratch by absolute image index, chunk c of every batch on stream c.  That is
    // only race-free while the chunk partition stays the same: another batch size cuts the images differently (256 ->
    // [0,85) [85,170) [170,256); 100 -> [0,33) [33,66) [66,100)), and chunk 1 of the new batch (stream 1) would overwrite
    // the scratch of images 33..66 that chunk 0 of the old one (stream 0) may still be reading.  So a change of batch
    // size, like a change of geometry, waits for the flight first.
    if (F.in_flight > 0 && (B.w != e->plan.w || B.h != e->plan.h || B.batch > e->scratch.batch_cap || B.cap != F.last.cap ||
                            B.batch != F.last.batch)) {
        if ((st = finish_device(e))) return st;   // scratch is rebuilt / re-partitioned: nothing may be in flight
    }
    if ((st = ensure_plan(e, B.w, B.h))) return st;
    if ((st = ensure_batch(e, B.batch))) return st;
    F.last = B;
    if ((st = begin_chunks(e, B.batch, B.h_imgs != nullptr, chunks))) return st;
    if ((st = stereo_guard_wait(e, chunks))) return st;
    for (int c = 0; c < chunks; ++c) {
        const int b0 = (int)((long long)B.batch * c / chunks), b1 = (int)((long long)B.batch * (c + 1) / chunks);
        if (b1 > b0 && (st = enqueue_chunk(e, B, b0, b1 - b0, e->str.q[c], c == 0))) return st;
    }
    e->tim.ms[6] = (float)chunks;
    ++F.in_flight;
    return AOS2_OK;
}

static int run_device(aos2_extractor *e, const BatchArgs &B)
{
    int st;
    if ((st = check_device_args(e, B))) return st;
    if (e->flight.in_flight > 0 && (st = finish_device(e))) return st;
    if ((st = enqueue_device(e, B))) return st;
    return finish_device(e);
}

// `launch(a, s)` -- one kernel over the last batch, whose slices are `a` -- `iters` times on the first stream, timed with events
template <class Launch>
static int bench_kernel(aos2_extractor *e, int iters, float *avg_ms, Launch launch)
{
    int st;
    if ((st = bind_device(e->par.device))) return st;
    if ((st = finish_device(e))) return st;   // batches enqueued asynchronously
    const ScratchAt a = scratch_at(e, 0);
    hipStream_t s = e->str.q[0];
    AOS2_HIP_CHECK(hipEventRecord(e->tim.ev[6], s));
    for (int i = 0; i < iters; ++i) launch(a, s);
    AOS2_HIP_CHECK(hipEventRecord(e->tim.ev[7], s));
    AOS2_HIP_CHECK(hipStreamSynchronize(s));
    AOS2_HIP_CHECK(hipEventElapsedTime(avg_ms, e->tim.ev[6], e->tim.ev[7]));
    *avg_ms /= iters;
    return AOS2_OK;
}

// LDS budget of an octree job: ~8 candidates per requested feature on level 0 (the busiest level), capped at the 64 KB a workgroup
// may take without opt-in; jobs that need more run over global scratch.  lds_override >= 0 replaces it (0: global path only).
// With `pair`: level g and level nlevels - 1 - g in one workgroup, each job in a slice of its own size (the default for batches).
static void octree_lds_budget(const Params &par, int lds_override, bool pair, Tuning &T)
{
    const int n0 = par.mnFeaturesPerLevel[0], nlevels = par.nlevels;
    T.oct_lds = lds_override >= 0 ? lds_override : (int)std::min<size_t>(oct_lds_bytes(8 * n0 + 256, n0), 65536);
    T.oct_pair = OctImageLayout{};
    if (T.oct_lds <= 0 || nlevels < 2 || !pair) return;
    int bytes[kMaxLevels], total = 0;
    for (int l = 0; l < nlevels; ++l) {
        const int nl = par.mnFeaturesPerLevel[l];
        bytes[l] = (int)up256(oct_lds_bytes(8 * nl + (l == 0 ? 256 : 128), nl));
        if (bytes[l] > T.oct_lds) bytes[l] = (T.oct_lds + 255) & ~255;   // (never more than the per-job form: larger jobs use global scratch)
    }
    for (int g2 = 0; g2 < (nlevels + 1) / 2; ++g2) {
        const int la = g2, lb = nlevels - 1 - g2;
        T.oct_pair.off[la] = 0; T.oct_pair.bytes[la] = bytes[la];
        int sum = bytes[la];
        if (lb != la) {
            T.oct_pair.off[lb] = bytes[la]; T.oct_pair.bytes[lb] = bytes[lb];
            sum += bytes[lb];
        }
        total = std::max(total, sum);
    }
    T.oct_pair.total = total <= 160 * 1024 ? total : 0;
}

// The six AOS2_* switches, read here and nowhere else; names, meanings, defaults and clamps: struct Tuning.
static void read_tuning(const Params &par, Tuning &T)
{
    if (const char *v = getenv("AOS2_FAST_LIST")) T.fast_list = std::max(264, atoi(v));
    if (const char *v = getenv("AOS2_PYRAMID")) T.pyr_levels = strcmp(v, "levels") == 0;
    const char *lds = getenv("AOS2_OCT_LDS"), *pair = getenv("AOS2_OCT_PAIR"), *group = getenv("AOS2_OCT_GROUP_LEVELS");
    if (group) T.group_levels = std::max(-1, atoi(group));
    octree_lds_budget(par, lds ? std::max(0, std::min(65536, atoi(lds))) : -1, !(pair && atoi(pair) == 0) && !group, T);
    if (const char *v = getenv("AOS2_CHUNKS")) T.chunks = std::max(0, std::min(kMaxStreams, atoi(v)));
}

}  // namespace aos2

// ------------------------------------------------------------------------------------------ C ABI
extern "C" {

const char *aos2_last_error(void) { return g_err.c_str(); }
const char *aos2_version(void) { return "aos2 0.1 (gfx950, HIP)"; }

int aos2_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int aos2_device_local_cpus(int device, char *buf, int cap)
{
    if (!buf || cap < 1) return AOS2_ERR_ARG;
    buf[0] = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
        (void)hipGetLastError();
        return AOS2_ERR_NO_DEVICE;
    }
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) {
        (void)hipGetLastError();
        return AOS2_OK;   // unknown: the empty list
    }
    for (char *c = bus; *c; ++c) *c = (char)tolower(*c);   // sysfs names are lower case
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/local_cpulist";
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return AOS2_OK;
    char line[4096] = {0};
    const bool got = fgets(line, sizeof(line), f) != nullptr;
    fclose(f);
    if (!got) return AOS2_OK;
    size_t len = strlen(line);
    while (len && (line[len - 1] == '\n' || line[len - 1] == ' ')) line[--len] = 0;
    if ((int)len + 1 > cap) return AOS2_ERR_CAPACITY;
    memcpy(buf, line, len + 1);
    return AOS2_OK;
}

int aos2_extractor_create(int nfeatures, float scale_factor, int nlevels, int ini_th_fast, int min_th_fast,
                          int device, aos2_extractor_t **out)
{
    if (!out) return AOS2_ERR_ARG;
    *out = nullptr;
    if (nfeatures <= 0 || nlevels < 1 || nlevels > kMaxLevels || !(scale_factor > 1.0f) || ini_th_fast < 1 ||
        min_th_fast < 1 || min_th_fast > ini_th_fast || ini_th_fast > 255) return bad_arg("bad extractor parameters");
    if (scale_factor > 2.0f) {  // the resize kernel stages <= 2.5x source windows in LDS
        set_error("scale factor %.3f > 2.0 is not supported", scale_factor);
        return AOS2_ERR_ARG;
    }
    aos2_extractor *e = new aos2_extractor();
    e->par.nfeatures = nfeatures;
    e->par.nlevels = nlevels;
    e->par.iniTh = ini_th_fast;
    e->par.minTh = min_th_fast;
    e->par.scaleFactor = scale_factor;
    e->par.device = device;
    build_host_tables(&e->par);
    read_tuning(e->par, e->tun);
    *out = e;
    return AOS2_OK;
}

void aos2_extractor_destroy(aos2_extractor_t *e)
{
    if (!e) return;
    if (e->str.ready) {
        (void)hipSetDevice(e->par.device);
        for (hipStream_t q : e->str.q) (void)hipStreamSynchronize(q);
        stereo_unpair(e);   // (the streams are drained: a partner's guard that names one has nothing left to order)
        e->plan.release();
        e->scratch.release();
        e->flight.release();
        e->host.release();
        e->stereo.release();
        for (hipEvent_t x : e->tim.ev) (void)hipEventDestroy(x);
        for (hipStream_t q : e->str.q) (void)hipStreamDestroy(q);
        for (hipEvent_t x : e->str.order_ev)
            if (x) (void)hipEventDestroy(x);
        for (hipEvent_t x : {e->guard.ev, e->stereo.t0, e->stereo.t1, e->str.input_ev, e->str.input_fan_ev})
            if (x) (void)hipEventDestroy(x);
    }
    delete e;
}

int aos2_extractor_levels(const aos2_extractor_t *e) { return e->par.nlevels; }
float aos2_extractor_scale_factor(const aos2_extractor_t *e) { return e->par.scaleFactor; }
const float *aos2_extractor_scale_factors(const aos2_extractor_t *e) { return e->par.mvScaleFactor; }
const float *aos2_extractor_inv_scale_factors(const aos2_extractor_t *e) { return e->par.mvInvScaleFactor; }
const float *aos2_extractor_sigma2(const aos2_extractor_t *e) { return e->par.mvLevelSigma2; }
const float *aos2_extractor_inv_sigma2(const aos2_extractor_t *e) { return e->par.mvInvLevelSigma2; }
const int *aos2_extractor_features_per_level(const aos2_extractor_t *e) { return e->par.mnFeaturesPerLevel; }
const int *aos2_extractor_umax(const aos2_extractor_t *e) { return e->par.umax; }
int aos2_extractor_max_keypoints(const aos2_extractor_t *e) { return e->par.max_kp; }
int aos2_extractor_max_keypoints_for(const aos2_extractor_t *e, int w, int h)
{
    if (!e) return 0;
    int cl = 0, tot = 0;
    keypoint_bounds(e->par, w, h, &cl, &tot);
    return tot;
}

int aos2_extractor_extract_batch_device(aos2_extractor_t *e, const uint8_t *d_imgs, int batch, int w, int h,
                                        int stride, size_t image_stride, aos2_keypoint_t *d_kps, uint8_t *d_desc,
                                        int cap, int32_t *d_n_out)
{
    return run_device(e, BatchArgs{d_imgs, batch, w, h, stride, image_stride, d_kps, d_desc, cap, d_n_out, nullptr, 0, 0, nullptr, nullptr});
}

int aos2_extractor_extract_batch_device_async(aos2_extractor_t *e, const uint8_t *d_imgs, int batch, int w, int h,
                                              int stride, size_t image_stride, aos2_keypoint_t *d_kps,
                                              uint8_t *d_desc, int cap, int32_t *d_n_out)
{
    return enqueue_device(e, BatchArgs{d_imgs, batch, w, h, stride, image_stride, d_kps, d_desc, cap, d_n_out, nullptr, 0, 0, nullptr, nullptr});
}

// fixed-size per-frame slots for the one exchange step of the sharded path:
// {int32 n; int32 pad[3]; KeyPoint[cap]; uint8 desc[cap][32]} rounded up to 16 B -- sharding.py's layout
__global__ __launch_bounds__(256) void pack_slots_kernel(const aos2_keypoint_t *__restrict__ kps, const uint8_t *__restrict__ desc,
                                                         const int32_t *__restrict__ n_out, int cap, uint8_t *__restrict__ slots,
                                                         size_t slot_bytes)
{
    const int b = blockIdx.y;
    uint4 *dst = reinterpret_cast<uint4 *>(slots + (size_t)b * slot_bytes);
    const int n = min(n_out[b], cap);
    const size_t words = slot_bytes / 16;
    const size_t kp_words = ((size_t)cap * 28) / 16;   // cap * 28 is a multiple of 16 for the capacities in use (checked by the host)
    const uint4 *ksrc = reinterpret_cast<const uint4 *>(kps + (size_t)b * cap);
    const uint4 *dsrc = reinterpret_cast<const uint4 *>(desc + (size_t)b * cap * 32);
    const size_t kp_used = ((size_t)n * 28 + 15) / 16, d_used = (size_t)n * 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (i == 0)
            v.x = (uint32_t)n;
        else if (i - 1 < kp_words) {
            if (i - 1 < kp_used) v = ksrc[i - 1];
        } else if (i - 1 - kp_words < d_used)
            v = dsrc[i - 1 - kp_words];
        dst[i] = v;
    }
}

int aos2_extractor_pack_slots(aos2_extractor_t *e, int batch, const aos2_keypoint_t *d_kps, const uint8_t *d_desc,
                              const int32_t *d_n, int cap, uint8_t *d_slots, size_t slot_bytes, void *hip_stream)
{
    if (!e || batch <= 0 || !d_kps || !d_desc || !d_n || !d_slots || cap <= 0 || ((size_t)cap * 28) % 16 != 0 ||
        slot_bytes % 16 != 0 || slot_bytes < 16 + (size_t)cap * 60)
        return bad_arg("bad argument (cap must be a multiple of 4, slot_bytes >= 16 + 60 * cap and a multiple of 16)");
    int st = aos2_extractor_stream_wait(e, hip_stream);
    if (st) return st;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(pack_slots_kernel, dim3(16, batch), dim3(256), 0, s, d_kps, d_desc, d_n, cap, d_slots, slot_bytes);
    AOS2_HIP_CHECK(hipGetLastError());
    return AOS2_OK;
}

int aos2_extractor_wait_for_stream(aos2_extractor_t *e, void *hip_stream)
{
    if (!e) return bad_arg();
    int st = init_device(e);
    if (st) return st;
    hipStream_t src = static_cast<hipStream_t>(hip_stream);
    if (!e->str.input_ev) AOS2_HIP_CHECK(hipEventCreateWithFlags(&e->str.input_ev, hipEventDisableTiming));
    AOS2_HIP_CHECK(hipEventRecord(e->str.input_ev, src));
    // the streams the last batch's chunks ran on wait now; a next batch cut into more chunks orders the others behind stream 0
    // (enqueue_device).  Streams that get no work are left alone: a recording (aos2_capture_begin) must not be joined by
    // streams that never return to it.
    // While `src` is being recorded only stream 0 joins: the batch behind this call may be cut into fewer chunks than the last one,
    // and a stream that joined a recording without getting work never returns to it (hipStreamEndCapture would fail).
    const int k = stream_is_capturing(src) ? 1 : std::max(1, std::min(kMaxStreams, e->str.last_chunks));
    for (int i = 0; i < k; ++i) AOS2_HIP_CHECK(hipStreamWaitEvent(e->str.q[i], e->str.input_ev, 0));
    e->str.input_waited = std::max(e->str.input_waited, k);
    return AOS2_OK;
}

int aos2_extractor_stream_wait(aos2_extractor_t *e, void *hip_stream)
{
    if (!e) return bad_arg();
    if (!e->str.ready) return AOS2_OK;   // nothing was ever enqueued
    int st = bind_device(e->par.device);
    if (st) return st;
    hipStream_t waiter = static_cast<hipStream_t>(hip_stream);
    const int used = std::max(1, std::min(kMaxStreams, e->str.used));
    for (int i = 0; i < used; ++i) {
        if (!e->str.order_ev[i]) AOS2_HIP_CHECK(hipEventCreateWithFlags(&e->str.order_ev[i], hipEventDisableTiming));
        if (e->str.q[i] == waiter) continue;   // (in order behind its own work already)
        AOS2_HIP_CHECK(hipEventRecord(e->str.order_ev[i], e->str.q[i]));
        AOS2_HIP_CHECK(hipStreamWaitEvent(waiter, e->str.order_ev[i], 0));
    }
    return AOS2_OK;
}

int aos2_extractor_wait(aos2_extractor_t *e)
{
    if (!e) return bad_arg();
    if (!e->str.ready) return AOS2_OK;
    int st = bind_device(e->par.device);
    if (st) return st;
    return finish_device(e);
}

int aos2_extractor_extract_batch(aos2_extractor_t *e, const uint8_t *imgs, int batch, int w, int h, int stride,
                                 size_t image_stride, aos2_keypoint_t *kps, uint8_t *desc, int cap, int32_t *n_out)
{
    if (!e || batch <= 0 || !n_out) return bad_arg();
    if (!imgs || w <= 0 || h <= 0) {  // empty image: silent return (:1046)
        for (int b = 0; b < batch; ++b) n_out[b] = 0;
        return AOS2_OK;
    }
    if (stride < w || cap <= 0 || !kps || !desc) return bad_arg();
    int st;
    if ((st = init_device(e))) return st;
    HostCall &H = e->host;
    if ((st = H.d_in.alloc((size_t)batch * w * h)) || (st = H.d_kps.alloc((size_t)batch * cap)) ||
        (st = H.d_desc.alloc((size_t)batch * cap * 32)) || (st = H.d_nout.alloc(batch)))
        return st;
    H.out_cap = cap;
    // uploads, kernels and downloads are pipelined per chunk on the chunk's stream (enqueue_chunk)
    st = run_device(e, BatchArgs{H.d_in.p, batch, w, h, w, (size_t)w * h, H.d_kps.p, H.d_desc.p, cap, H.d_nout.p, imgs, stride, image_stride,
                                 kps, desc});
    if (st == AOS2_OK || st == AOS2_ERR_CAPACITY) {
        for (int b = 0; b < batch; ++b) n_out[b] = e->scratch.h_nout.p[b];
    }
    return st;
}

int aos2_host_alloc(void **p, size_t bytes)
{
    if (!p || bytes == 0) return bad_arg();
    *p = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return AOS2_FAIL(AOS2_ERR_NO_DEVICE, "no HIP device: page-locked host memory needs the GPU runtime");
    AOS2_HIP_CHECK(hipHostMalloc(p, bytes, hipHostMallocDefault));
    return AOS2_OK;
}

int aos2_host_free(void *p)
{
    if (!p) return AOS2_OK;
    AOS2_HIP_CHECK(hipHostFree(p));
    return AOS2_OK;
}

int aos2_extractor_extract(aos2_extractor_t *e, const uint8_t *img, int w, int h, int stride, aos2_keypoint_t *kps,
                           uint8_t *desc, int cap, int *n_out)
{
    int32_t n = 0;
    const int st = aos2_extractor_extract_batch(e, img, 1, w, h, stride, (size_t)stride * (h > 0 ? h : 0), kps, desc,
                                                cap, &n);
    if (n_out) *n_out = n;
    return st;
}

// ---------------------------------------------------------------------------------------------
// Frame::ComputeStereoMatches (src/Frame.cc:495-669): the two extractors keep mvImagePyramid of the
// last call in HBM; kernels are in stereo.hip.
static void fill_view(aos2_extractor *e, PyrView &v)
{
    static_cast<ImagePlanes &>(v) = scratch_at(e, 0).planes;
    v.nlevels = e->par.nlevels;
    for (int l = 0; l < e->par.nlevels; ++l) {
        const LevelDev &L = e->plan.levels[l];
        v.w[l] = L.w; v.h[l] = L.h; v.pitch[l] = L.pitch; v.off[l] = L.off;
        v.scale[l] = e->par.mvScaleFactor[l];
        v.inv_scale[l] = e->par.mvInvScaleFactor[l];
    }
}

// The argument check of ComputeStereoMatches on images [first_image, first_image + batch); form_ok = the calling form's own rules.
static int check_stereo_args(const aos2_extractor *l, const aos2_extractor *r, int first_image, int batch, float mb, bool form_ok)
{
    if (!l || !r || l->plan.levels.empty() || r->plan.levels.empty() || l->flight.last.batch <= 0 || r->flight.last.batch <= 0)
        return bad_arg("ComputeStereoMatches: both extractors must hold the pyramids of an extract call");
    if (l->par.device != r->par.device || l->par.nlevels != r->par.nlevels || l->par.nlevels > kStereoMaxLevels ||
        l->par.scaleFactor != r->par.scaleFactor || l->plan.w != r->plan.w || l->plan.h != r->plan.h)
        return bad_arg("ComputeStereoMatches: left/right extractors differ (device, levels, scale or image size)");
    if (!form_ok || first_image < 0 || batch <= 0 || batch > l->flight.last.batch - first_image ||
        batch > r->flight.last.batch - first_image || !(mb > 0)) return bad_arg("ComputeStereoMatches: bad argument");
    return AOS2_OK;
}

// The keypoint records the kernels may be given (aos2.h, "domain of ComputeStereoMatches"): with them the 11 x 11 left window
// (:592) and the 11 x 21 right window (:609) stay inside mvImagePyramid[levelL] and both scale tables are indexed in range.  The
// reference throws from rowRange / colRange at the same records.  Host arrays only: the device-resident forms state it as
// their precondition.
static int check_stereo_keypoints(const aos2_extractor *l, const aos2_keypoint_t *kl, int n_left, const aos2_keypoint_t *kr,
                                  int n_right)
{
    const int nlevels = l->par.nlevels, rows = l->plan.levels[0].h;
    const float *inv = l->par.mvInvScaleFactor;
    for (int i = 0; i < n_left; ++i) {
        const aos2_keypoint_t &k = kl[i];
        if (k.octave < 0 || k.octave >= nlevels || !std::isfinite(k.x) || !std::isfinite(k.y))
            return AOS2_FAIL(AOS2_ERR_ARG, "ComputeStereoMatches: left keypoint %d: octave out of range or position not finite", i);
        const LevelDev &L = l->plan.levels[k.octave];
        const float cu = roundf(k.x * inv[k.octave]), cv = roundf(k.y * inv[k.octave]);
        if (!(k.y > -1.0f && k.y < (float)rows) || !(cv >= 5.0f && cv <= (float)(L.h - 6)) || !(cu >= 5.0f && cu <= (float)(L.w - 6)))
            return AOS2_FAIL(AOS2_ERR_ARG, "ComputeStereoMatches: left keypoint %d: the 11 x 11 window leaves level %d", i, k.octave);
    }
    for (int i = 0; i < n_right; ++i) {
        const aos2_keypoint_t &k = kr[i];
        if (k.octave < 0 || k.octave >= nlevels || !std::isfinite(k.y))
            return AOS2_FAIL(AOS2_ERR_ARG, "ComputeStereoMatches: right keypoint %d: octave out of range or y not finite", i);
        for (int lv = std::max(k.octave - 1, 0); lv <= std::min(k.octave + 1, nlevels - 1); ++lv) {
            const float cu = roundf(k.x * inv[lv]);   // < 0: refused by iniu (:604); >= 10: cuR0 - 10 is a column of the plane
            if (cu >= 0.0f && cu < 10.0f)
                return AOS2_FAIL(AOS2_ERR_ARG, "ComputeStereoMatches: right keypoint %d: the search window leaves level %d", i, lv);
        }
    }
    return AOS2_OK;
}

static int stereo_run(aos2_extractor *l, aos2_extractor *r, int first_image, int batch, const aos2_keypoint_t *d_kpl,
                      const uint8_t *d_dl, const int32_t *d_nl, const aos2_keypoint_t *d_kpr, const uint8_t *d_dr,
                      const int32_t *d_nr, int cap, int max_n_left, float mb, float mbf, float *d_ur, float *d_depth, bool sync = true)
{
    int st;
    if ((st = l->stereo.sad.alloc((size_t)batch * cap))) return st;
    StereoArgs a;
    fill_view(l, a.L);
    fill_view(r, a.R);
    a.first_image_l = a.first_image_r = first_image;
    a.kp_l = d_kpl; a.kp_r = d_kpr; a.desc_l = d_dl; a.desc_r = d_dr; a.n_l = d_nl; a.n_r = d_nr;
    a.cap = cap; a.batch = batch; a.mb = mb; a.mbf = mbf;
    a.u_right = d_ur; a.depth = d_depth; a.sad = l->stereo.sad.p;
    a.rows = a.L.h[0];
    a.row_cap = cap * stereo_row_span(a.L);
    if ((st = l->stereo.rows.alloc((size_t)batch * ((size_t)a.rows + 1 + (size_t)a.row_cap)))) return st;
    a.row_off = l->stereo.rows.p;
    a.row_idx = l->stereo.rows.p + (size_t)batch * ((size_t)a.rows + 1);
    // (events of its own: ev[0..5] are the stage timings of the extraction, which finish_device() reads)
    if (!l->stereo.t0) {
        AOS2_HIP_CHECK(hipEventCreate(&l->stereo.t0));
        AOS2_HIP_CHECK(hipEventCreate(&l->stereo.t1));
    }
    for (aos2_extractor *x : {l, r})
        if (!x->guard.ev) AOS2_HIP_CHECK(hipEventCreateWithFlags(&x->guard.ev, hipEventDisableTiming));
    AOS2_HIP_CHECK(hipEventRecord(l->stereo.t0, l->str.q[0]));
    if ((st = launch_stereo(a, max_n_left, l->str.q[0]))) return st;
    AOS2_HIP_CHECK(hipEventRecord(l->stereo.t1, l->str.q[0]));
    for (aos2_extractor *x : {l, r}) {   // the next extraction of either eye is ordered behind these kernels on all its streams
        AOS2_HIP_CHECK(hipEventRecord(x->guard.ev, l->str.q[0]));
        x->guard.armed = true;
        x->guard.captured = stream_is_capturing(l->str.q[0]);
        x->guard.stream = l->str.q[0];
    }
    if (l != r && l->guard.peer != r) {   // a new pairing: each eye leaves the partner it had (stereo_unpair)
        stereo_unpair(l);
        stereo_unpair(r);
        l->guard.peer = r;
        r->guard.peer = l;
    }
    if (!sync) return AOS2_OK;
    AOS2_HIP_CHECK(hipStreamSynchronize(l->str.q[0]));
    AOS2_HIP_CHECK(hipEventElapsedTime(&l->stereo.ms, l->stereo.t0, l->stereo.t1));
    return AOS2_OK;
}

// The stereo Frame constructor's pipeline without a host wait (src/Frame.cc:57-113: the two ExtractORB threads are joined, then
// ComputeStereoMatches runs): left's first stream waits -- on the device -- for every stream of both extractors' batches in
// flight, the stereo kernels are enqueued behind, and whatever orders itself behind `left` afterwards (aos2_extractor_stream_wait,
// aos2_frames_build_stereo, aos2_extractor_wait) is ordered behind them.
int aos2_compute_stereo_matches_device_async(aos2_extractor_t *left, aos2_extractor_t *right, int batch,
                                             const aos2_keypoint_t *d_kp_left, const uint8_t *d_desc_left,
                                             const int32_t *d_n_left, const aos2_keypoint_t *d_kp_right,
                                             const uint8_t *d_desc_right, const int32_t *d_n_right, int cap, float mb,
                                             float mbf, float *d_u_right, float *d_depth)
{
    const bool form_ok = d_kp_left && d_desc_left && d_n_left && d_kp_right && d_desc_right && d_n_right && d_u_right && d_depth &&
                         cap > 0 && left != right;
    int st;
    if ((st = check_stereo_args(left, right, 0, batch, mb, form_ok))) return st;
    if ((st = bind_device(left->par.device))) return st;
    if ((st = aos2_extractor_stream_wait(left, left->str.q[0])) || (st = aos2_extractor_stream_wait(right, left->str.q[0]))) return st;
    return stereo_run(left, right, 0, batch, d_kp_left, d_desc_left, d_n_left, d_kp_right, d_desc_right, d_n_right, cap,
                      cap, mb, mbf, d_u_right, d_depth, false);
}

int aos2_compute_stereo_matches_device(aos2_extractor_t *left, aos2_extractor_t *right, int batch,
                                       const aos2_keypoint_t *d_kp_left, const uint8_t *d_desc_left,
                                       const int32_t *d_n_left, const aos2_keypoint_t *d_kp_right,
                                       const uint8_t *d_desc_right, const int32_t *d_n_right, int cap, float mb,
                                       float mbf, float *d_u_right, float *d_depth)
{
    const bool form_ok = d_kp_left && d_desc_left && d_n_left && d_kp_right && d_desc_right && d_n_right && d_u_right && d_depth &&
                         cap > 0;
    int st;
    if ((st = check_stereo_args(left, right, 0, batch, mb, form_ok))) return st;
    if ((st = bind_device(left->par.device))) return st;
    if ((st = finish_device(left)) || (st = finish_device(right))) return st;
    return stereo_run(left, right, 0, batch, d_kp_left, d_desc_left, d_n_left, d_kp_right, d_desc_right, d_n_right, cap,
                      cap, mb, mbf, d_u_right, d_depth);
}

int aos2_compute_stereo_matches(aos2_extractor_t *left, aos2_extractor_t *right, int image,
                                const aos2_keypoint_t *kp_left, const uint8_t *desc_left, int n_left,
                                const aos2_keypoint_t *kp_right, const uint8_t *desc_right, int n_right, float mb,
                                float mbf, float *u_right, float *depth)
{
    int st;
    const bool form_ok = n_left >= 0 && n_right >= 0 && (n_left == 0 || (kp_left && desc_left && u_right && depth)) &&
                         (n_right == 0 || (kp_right && desc_right));
    if ((st = check_stereo_args(left, right, image, 1, mb, form_ok))) return st;
    if ((st = check_stereo_keypoints(left, kp_left, n_left, kp_right, n_right))) return st;
    if (n_left == 0) return AOS2_OK;
    if ((st = bind_device(left->par.device))) return st;
    if ((st = finish_device(left)) || (st = finish_device(right))) return st;
    aos2_extractor *e = left;
    const int cap = ((n_left > n_right ? n_left : n_right) + 3) & ~3;  // keeps the descriptor blocks 16-byte aligned
    const size_t kb = sizeof(aos2_keypoint_t) * (size_t)cap, db = (size_t)cap * 32;
    // one upload block: kpL | kpR | descL | descR | nL nR ; one download block: uRight | depth
    const size_t o_kr = kb, o_dl = 2 * kb, o_dr = 2 * kb + db, o_n = 2 * kb + 2 * db, o_out = o_n + 16;
    const size_t total = o_out + 2 * sizeof(float) * (size_t)cap;
    if ((st = e->stereo.io.alloc(total))) return st;
    if ((st = e->stereo.host.alloc(total))) return st;
    uint8_t *hp = e->stereo.host.p;
    memcpy(hp, kp_left, sizeof(aos2_keypoint_t) * (size_t)n_left);
    if (n_right) memcpy(hp + o_kr, kp_right, sizeof(aos2_keypoint_t) * (size_t)n_right);
    memcpy(hp + o_dl, desc_left, (size_t)n_left * 32);
    if (n_right) memcpy(hp + o_dr, desc_right, (size_t)n_right * 32);
    int32_t nn[2] = {n_left, n_right};
    memcpy(hp + o_n, nn, sizeof(nn));
    AOS2_HIP_CHECK(hipMemcpyAsync(e->stereo.io.p, hp, o_out, hipMemcpyHostToDevice, e->str.q[0]));
    uint8_t *dp = e->stereo.io.p;
    st = stereo_run(left, right, image, 1, (const aos2_keypoint_t *)dp, dp + o_dl, (const int32_t *)(dp + o_n),
                    (const aos2_keypoint_t *)(dp + o_kr), dp + o_dr, (const int32_t *)(dp + o_n) + 1, cap, n_left, mb,
                    mbf, (float *)(dp + o_out), (float *)(dp + o_out) + cap);
    if (st) return st;
    AOS2_HIP_CHECK(hipMemcpyAsync(hp + o_out, dp + o_out, 2 * sizeof(float) * (size_t)cap, hipMemcpyDeviceToHost, e->str.q[0]));
    AOS2_HIP_CHECK(hipStreamSynchronize(e->str.q[0]));
    memcpy(u_right, hp + o_out, sizeof(float) * (size_t)n_left);
    memcpy(depth, hp + o_out + sizeof(float) * (size_t)cap, sizeof(float) * (size_t)n_left);
    return AOS2_OK;
}

float aos2_compute_stereo_matches_last_device_ms(const aos2_extractor_t *left) { return left ? left->stereo.ms : 0.0f; }

int aos2_extractor_pyramid_level_size(const aos2_extractor_t *e, int level, int *w, int *h)
{
    if (!e || level < 0 || level >= e->par.nlevels || e->plan.levels.empty()) return bad_arg("no pyramid available");
    if (w) *w = e->plan.levels[level].w;
    if (h) *h = e->plan.levels[level].h;
    return AOS2_OK;
}

int aos2_extractor_pyramid_level(aos2_extractor_t *e, int image, int level, int border, uint8_t *dst, int dst_stride)
{
    if (!e || !dst || level < 0 || level >= e->par.nlevels || e->plan.levels.empty() || image < 0 ||
        image >= e->flight.last.batch || border < 0 || border > 64) return bad_arg("bad argument / no pyramid available");
    int st;
    if ((st = bind_device(e->par.device))) return st;
    if ((st = finish_device(e))) return st;   // batches enqueued asynchronously
    const LevelDev &L = e->plan.levels[level];
    if (dst_stride < L.w + 2 * border) return AOS2_ERR_ARG;
    uint8_t *interior = dst + (size_t)border * dst_stride + border;
    const ImagePlanes pl = scratch_at(e, image).planes;
    const uint8_t *srcp = level == 0 ? pl.img0 : pl.pyr + L.off;
    const size_t srcpitch = level == 0 ? (size_t)pl.pitch0 : (size_t)L.pitch;
    AOS2_HIP_CHECK(hipMemcpy2DAsync(interior, (size_t)dst_stride, srcp, srcpitch, (size_t)L.w, (size_t)L.h,
                                    hipMemcpyDeviceToHost, e->str.q[0]));
    AOS2_HIP_CHECK(hipStreamSynchronize(e->str.q[0]));
    if (border > 0) {  // cv::copyMakeBorder(BORDER_REFLECT_101), :1122-1128
        auto refl = [](int p, int n) {
            while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
            return p;
        };
        for (int y = -border; y < L.h + border; ++y) {
            const uint8_t *srow = interior + (ptrdiff_t)refl(y, L.h) * dst_stride;
            uint8_t *drow = interior + (ptrdiff_t)y * dst_stride;
            for (int x = -border; x < L.w + border; ++x) {
                if (y >= 0 && y < L.h && x >= 0 && x < L.w) continue;
                drow[x] = srow[refl(x, L.w)];
            }
        }
    }
    return AOS2_OK;
}

int aos2_extractor_debug_candidates(aos2_extractor_t *e, int image, int level, int16_t *xs, int16_t *ys,
                                    uint8_t *score, int cap, int *n)
{
    if (!e || !n || level < 0 || level >= e->par.nlevels || image < 0 || image >= e->flight.last.batch) return bad_arg();
    int st;
    if ((st = bind_device(e->par.device))) return st;
    if ((st = finish_device(e))) return st;   // batches enqueued asynchronously
    const ScratchAt a = scratch_at(e, image);
    // per-level lists, written by the octree jobs at the level's first slot
    int32_t cnt = 0;
    AOS2_HIP_CHECK(hipMemcpy(&cnt, a.gather.level_cnt + level, sizeof(cnt), hipMemcpyDeviceToHost));
    const int first = e->plan.cells[e->plan.level_cell_begin[level]].slot_off;
    *n = cnt;
    if (!xs || !ys || !score) return AOS2_OK;
    if (cnt > cap) return AOS2_ERR_CAPACITY;
    std::vector<uint32_t> tmp(cnt > 0 ? cnt : 1);
    if (cnt > 0)
        AOS2_HIP_CHECK(hipMemcpy(tmp.data(), a.dense + first, sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost));
    for (int i = 0; i < cnt; ++i) {
        xs[i] = (int16_t)(tmp[i] & 0xfff);
        ys[i] = (int16_t)((tmp[i] >> 12) & 0xfff);
        score[i] = (uint8_t)(tmp[i] >> 24);
    }
    return AOS2_OK;
}

int aos2_extractor_set_chunks(aos2_extractor_t *e, int chunks)
{
    if (!e || chunks < 0 || chunks > kMaxStreams) return AOS2_ERR_ARG;
    e->tun.chunks = chunks;
    return AOS2_OK;
}

int aos2_extractor_last_timing(const aos2_extractor_t *e, float *ms, int n)
{
    if (!e || !ms) return AOS2_ERR_ARG;
    for (int i = 0; i < n && i < 8; ++i) ms[i] = e->tim.ms[i];
    return AOS2_OK;
}

int aos2_extractor_bench_fast(aos2_extractor_t *e, int iters, float *avg_ms)
{
    if (!e || !avg_ms || iters <= 0 || e->flight.last.batch <= 0) return bad_arg("bench_fast needs a previous batch");
    const Plan &P = e->plan;
    return bench_kernel(e, iters, avg_ms, [&](const ScratchAt &a, hipStream_t s) {
        launch_fast(a.planes, P.d_cells, (int)P.cells.size(), e->par.iniTh, e->par.minTh, P.fast, a.slots, P.slot_total, a.cell_cnt,
                    e->flight.last.batch, s);
    });
}

int aos2_extractor_bench_describe(aos2_extractor_t *e, int iters, float *avg_ms)
{
    if (!e || !avg_ms || iters <= 0 || e->flight.last.batch <= 0 || !e->host.d_kps.p || e->host.out_cap <= 0)
        return bad_arg("bench_describe needs a previous host-API batch");
    const HostCall *H = &e->host;
    return bench_kernel(e, iters, avg_ms, [&](const ScratchAt &a, hipStream_t s) {
        launch_describe(a.planes, e->plan.d_levels, e->par.nlevels, a.sel, H->d_kps.p, H->d_desc.p, H->out_cap, H->d_nout.p,
                        e->flight.last.batch, e->par.umax_nibbles, e->flight.d_status.p, s);
    });
}

int aos2_debug_extractor_plan(const aos2_extractor_t *e, int w, int h, int64_t *levels, int32_t *cells, int cell_cap, int *n_cells,
                              int64_t *totals)
{
    if (!e || !levels || !n_cells || !totals) return bad_arg();
    Plan P;
    if (int st = make_plan(e->par, e->tun, w, h, P)) return st;
    for (size_t l = 0; l < P.levels.size(); ++l) {
        const LevelDev &L = P.levels[l];
        const int64_t v[4] = {L.w, L.h, L.pitch, (int64_t)L.off};
        memcpy(levels + 4 * l, v, sizeof(v));
    }
    *n_cells = (int)P.cells.size();
    totals[0] = (int64_t)P.pyr_bytes;
    totals[1] = (int64_t)P.slot_total;
    if (!cells) return AOS2_OK;
    if (*n_cells > cell_cap) return AOS2_ERR_CAPACITY;
    for (size_t c = 0; c < P.cells.size(); ++c) {
        const CellDev &C = P.cells[c];
        const int32_t v[6] = {C.level, C.vx0, C.vy0, C.cw, C.ch, C.slot_off};
        memcpy(cells + 6 * c, v, sizeof(v));
    }
    return AOS2_OK;
}

}  // extern "C"
