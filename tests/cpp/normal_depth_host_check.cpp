// TEST INFRASTRUCTURE: the host side of MapPoint::UpdateNormalAndDepth (active-orb-slam2_amd/csrc/normal_depth.h: the argument checks,
// the arithmetic and the serial loop that aos2_debug_update_normal_depth_host runs) as a stand-alone program, so that it can be built
// with -fsanitize=address,undefined and run on the CPU.  Seeded random graphs and batches with unknown, bad and repeated rows,
// reference keyframes with and without features, room for the per-observation outputs that matches and that does not; each output
// array is allocated at EXACTLY its size (a write behind one is a heap overflow the sanitizer reports) and preset, so that what a
// point that is not updated leaves behind shows; the values are checked against a second computation written here.  Then the
// refusals.  Exit status 0 and "ok" on success.
#include "../../active-orb-slam2_amd/csrc/normal_depth.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace aos2;

static int failures = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("line %d: %s\n", __LINE__, #c);                \
            ++failures;                                                \
        }                                                              \
    } while (0)

static bool same(float a, float b) { return !std::memcmp(&a, &b, 4) || (a != a && b != b); }
static float unit(std::mt19937 &rng) { return (float)(rng() % 20001) / 2000.0f - 5.0f; }

struct Graph {
    std::vector<uint8_t> point_bad;
    std::vector<int32_t> obs_off, obs_kf, obs_idx, kf_mp_off;
    std::vector<int8_t> kf_octave;
    LmGraph G = {};
    Graph(std::mt19937 &rng, int nk, int np, int n_levels)
    {
        kf_mp_off.push_back(0);
        for (int k = 0; k < nk; ++k) {
            const int nf = (int)(rng() % 5);
            for (int f = 0; f < nf; ++f) kf_octave.push_back((int8_t)((int)(rng() % (n_levels + 2)) - 1));   // -1 and n_levels: outside
            kf_mp_off.push_back((int32_t)kf_octave.size());
        }
        obs_off.push_back(0);
        for (int p = 0; p < np; ++p) {
            point_bad.push_back(rng() % 10 == 0);
            for (int k = 0; k < nk; ++k) {
                const int nf = kf_mp_off[k + 1] - kf_mp_off[k];
                if (nf == 0 || rng() % 3) continue;
                obs_kf.push_back(k);
                obs_idx.push_back((int32_t)(rng() % nf));
            }
            obs_off.push_back((int32_t)obs_kf.size());
        }
        G.n_points = np; G.n_kfs = nk;
        G.point_bad = point_bad.data(); G.obs_off = obs_off.data(); G.obs_kf = obs_kf.data();
        G.kf_mp_off = kf_mp_off.data(); G.obs_idx = obs_idx.data(); G.kf_octave = kf_octave.data();
    }
};

static void run_case(std::mt19937 &rng)
{
    const int nk = 1 + (int)(rng() % 20), np = (int)(rng() % 30), n = (int)(rng() % 12), n_levels = 1 + (int)(rng() % 8);
    const Graph g(rng, nk, np, n_levels);
    std::vector<int32_t> point(n), ref_kf(n), term_off(n + 1, 0);
    std::vector<float> xyz(3 * (size_t)n), centre(3 * (size_t)nk), scale(n_levels);
    for (float &v : xyz) v = unit(rng);
    for (float &v : centre) v = unit(rng);
    for (int l = 0; l < n_levels; ++l) scale[l] = 1.0f + 0.2f * (float)l;
    for (int i = 0; i < n; ++i) {
        point[i] = (int32_t)(rng() % (np + 2));
        ref_kf[i] = (int32_t)(rng() % nk);
        const int len = point[i] < np ? g.obs_off[point[i] + 1] - g.obs_off[point[i]] : 0;
        if (len && rng() % 4 == 0)   // now and then on a camera centre
            for (int c = 0; c < 3; ++c) xyz[3 * (size_t)i + c] = centre[3 * (size_t)g.obs_kf[g.obs_off[point[i]]] + c];
        term_off[i + 1] = term_off[i] + len + (rng() % 4 == 0);
    }
    const bool with_terms = rng() % 2;
    const float S = -7.0f;
    std::vector<uint8_t> status(n, 255);
    std::vector<float> normal(3 * (size_t)n, S), mn(n, S), mx(n, S), mean(n, S), sd(n, S), up(n, S), lo(n, S), maxr(n, S), minr(n, S),
        tu(with_terms ? 3 * (size_t)term_off[n] : 0, S), tt(with_terms ? (size_t)term_off[n] : 0, S);
    std::vector<int32_t> n_terms(n, -7);
    aos2_normal_depth_t a = {};
    a.n = n; a.point = point.data(); a.xyz = xyz.data(); a.ref_kf = ref_kf.data(); a.kf_center = centre.data();
    a.n_levels = n_levels; a.scale = scale.data(); a.rows_form = (int)(rng() % 2); a.term_off = with_terms ? term_off.data() : nullptr;
    a.status = status.data(); a.normal = normal.data(); a.min_dist = mn.data(); a.max_dist = mx.data(); a.theta_mean = mean.data();
    a.theta_std = sd.data(); a.n_terms = n_terms.data(); a.upper = up.data(); a.lower = lo.data(); a.max_range = maxr.data();
    a.min_range = minr.data(); a.term_unit = tu.empty() ? nullptr : tu.data(); a.term_theta = tt.empty() ? nullptr : tt.data();
    if (rng() % 5 == 0) a.normal = a.upper = a.theta_std = nullptr;   // outputs that are not wanted
    static int32_t none;
    static float nonef;
    if (!n) {   // (a zero-length std::vector may hand out NULL)
        a.point = a.ref_kf = &none;
        a.xyz = &nonef;
    }
    char why[200] = "";
    if (nd_check(a, nk, why, sizeof why)) {
        std::printf("a valid case was refused: %s\n", why);
        ++failures;
        return;
    }
    nd_host_run(g.G, a);
    for (int i = 0; i < n; ++i) {
        const int p = point[i];
        const int e0 = p < np ? g.obs_off[p] : 0, len = p < np ? g.obs_off[p + 1] - e0 : 0;
        int want = AOS2_ND_UPDATED, idx = 0;
        for (int j = 0; j < len; ++j)
            if (g.obs_kf[e0 + j] == ref_kf[i]) idx = g.obs_idx[e0 + j];
        const int f0 = g.kf_mp_off[ref_kf[i]], nf = g.kf_mp_off[ref_kf[i] + 1] - f0;
        if (p >= np) want = AOS2_ND_UNKNOWN;
        else if (g.point_bad[p]) want = AOS2_ND_BAD;
        else if (len == 0) want = AOS2_ND_NO_OBS;
        else if (idx >= nf || g.kf_octave[f0 + idx] < 0 || g.kf_octave[f0 + idx] >= n_levels) want = AOS2_ND_REF_UNUSABLE;
        EXPECT(status[i] == want);
        const bool room = with_terms && term_off[i + 1] - term_off[i] == len;
        if (want != AOS2_ND_UPDATED) {   // everything as it was
            EXPECT(mn[i] == S && mx[i] == S && mean[i] == S && sd[i] == S && lo[i] == S && maxr[i] == S && minr[i] == S && n_terms[i] == -7);
            if (a.normal) EXPECT(normal[3 * (size_t)i] == S && normal[3 * (size_t)i + 2] == S);
            for (int j = term_off[i]; with_terms && j < term_off[i + 1]; ++j) EXPECT(tt[j] == S && tu[3 * (size_t)j + 1] == S);
            continue;
        }
        // the second computation: the same conventions, written out again
        const float *P = &xyz[3 * (size_t)i];
        float acc[3] = {0.0f, 0.0f, 0.0f};
        double tsum = 0.0;
        std::vector<float> th(len);
        for (int j = 0; j < len; ++j) {
            const float *O = &centre[3 * (size_t)g.obs_kf[e0 + j]];
            const float d[3] = {P[0] - O[0], P[1] - O[1], P[2] - O[2]};
            const double s = ((double)d[0] * d[0] + (double)d[1] * d[1]) + (double)d[2] * d[2];
            const float inv = (float)(1.0 / std::sqrt(s));
            th[j] = (float)std::atan2((double)d[0], (double)d[2]);
            for (int c = 0; c < 3; ++c) {
                const float u = d[c] * inv;
                acc[c] = acc[c] + u;
                if (room) EXPECT(same(tu[3 * (size_t)(term_off[i] + j) + c], u));
            }
            if (room) EXPECT(same(tt[term_off[i] + j], th[j]));
            tsum += (double)th[j];
        }
        if (!room)
            for (int j = term_off[i]; with_terms && j < term_off[i + 1]; ++j) EXPECT(tt[j] == S && tu[3 * (size_t)j] == S);
        const float k = (float)(1.0 / (double)len);
        if (a.normal)
            for (int c = 0; c < 3; ++c) EXPECT(same(normal[3 * (size_t)i + c], acc[c] * k));
        const float *R = &centre[3 * (size_t)ref_kf[i]];
        const float r[3] = {P[0] - R[0], P[1] - R[1], P[2] - R[2]};
        const float dist = (float)std::sqrt(((double)r[0] * r[0] + (double)r[1] * r[1]) + (double)r[2] * r[2]);
        const float wmax = dist * scale[g.kf_octave[f0 + idx]], wmin = wmax / scale[n_levels - 1];
        EXPECT(same(mx[i], wmax) && same(mn[i], wmin) && n_terms[i] == len);
        const float m = (float)tsum / (float)len;
        double sq = 0.0;
        for (int j = 0; j < len; ++j) {
            const float diff = th[j] - m;
            sq += (double)(diff * diff);
        }
        const float sdev = std::sqrt((float)sq / (float)len);
        EXPECT(same(mean[i], m));
        if (a.theta_std) EXPECT(same(sd[i], sdev));
        EXPECT(same(maxr[i], 1.2f * wmax) && same(minr[i], 0.8f * wmin));
        float wlo;
        if (a.rows_form == AOS2_ND_ROWS_PLANNING) {
            const float iv = sdev * 2.5 < 30.0 / 57.3 ? (float)(30.0 / 57.3) : (float)(sdev * 2.5);
            wlo = m - iv;
        } else {
            const double iv = sdev * 2.5 < 10.0 / 57.3 ? 10.0 / 57.3 : sdev * 2.5;
            wlo = (float)(m - iv);
        }
        EXPECT(same(lo[i], wlo));
    }
}

static void refusals()
{
    int32_t point[2] = {0, 5}, ref_kf[2] = {0, 1}, term_off[3] = {0, 1, 1};
    float xyz[6] = {0}, centre[6] = {0}, scale[2] = {1.0f, 1.2f}, out[8];
    aos2_normal_depth_t ok = {};
    ok.n = 2; ok.point = point; ok.xyz = xyz; ok.ref_kf = ref_kf; ok.kf_center = centre; ok.n_levels = 2; ok.scale = scale;
    ok.rows_form = AOS2_ND_ROWS_TRACKING;
    char why[200];
    EXPECT(!nd_check(ok, 2, why, sizeof why));
    aos2_normal_depth_t a = ok;
    a.n = -1; EXPECT(nd_check(a, 2, why, sizeof why));
    a = ok; a.n_levels = 0; EXPECT(nd_check(a, 2, why, sizeof why));
    a = ok; a.rows_form = 2; EXPECT(nd_check(a, 2, why, sizeof why));
    a = ok; a.rows_form = -1; EXPECT(nd_check(a, 2, why, sizeof why));
    a = ok; a.point = nullptr; EXPECT(nd_check(a, 2, why, sizeof why));
    a = ok; a.xyz = nullptr; EXPECT(nd_check(a, 2, why, sizeof why));
    a = ok; a.ref_kf = nullptr; EXPECT(nd_check(a, 2, why, sizeof why));
    a = ok; a.kf_center = nullptr; EXPECT(nd_check(a, 2, why, sizeof why));
    a = ok; a.scale = nullptr; EXPECT(nd_check(a, 2, why, sizeof why));
    a = ok; a.term_unit = out; EXPECT(nd_check(a, 2, why, sizeof why));
    a = ok; a.term_theta = out; EXPECT(nd_check(a, 2, why, sizeof why));
    a.term_off = term_off; EXPECT(!nd_check(a, 2, why, sizeof why));
    term_off[0] = 1; EXPECT(nd_check(a, 2, why, sizeof why));
    term_off[0] = 0; term_off[2] = 0; EXPECT(nd_check(a, 2, why, sizeof why));
    a = ok; ref_kf[1] = 2; EXPECT(nd_check(a, 2, why, sizeof why));
    ref_kf[1] = -1; EXPECT(nd_check(a, 2, why, sizeof why));
    ref_kf[1] = 1; point[0] = -1; EXPECT(nd_check(a, 2, why, sizeof why));
    char tiny[8];
    EXPECT(nd_check(a, 2, tiny, sizeof tiny) && tiny[7] == 0);   // (the reason is cut to the buffer)
    a.n = 0; a.point = nullptr; a.xyz = nullptr; a.ref_kf = nullptr; EXPECT(!nd_check(a, 2, why, sizeof why));   // n == 0 reads nothing
}

int main()
{
    std::mt19937 rng(20241021);
    for (int i = 0; i < 3000; ++i) run_case(rng);
    refusals();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
