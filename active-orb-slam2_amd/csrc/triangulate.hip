// The host-pointer form of the loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:290-436; include/aos2.h:
// aos2_triangulate_matches): one (KF1, KF2) pair whose matches the caller lists, on the matcher's handle.  The arithmetic is
// csrc/triangulate.h, shared with the resident-batch form (frames_keyframe.hip) and the host tap.
#include "matcher_handle.h"
#include "triangulate.h"

namespace aos2 {

// the host-pointer form: one (KF1, KF2) pair, thread = match
__global__ __launch_bounds__(256) void triangulate_list_kernel(const aos2_triang_geom_t *__restrict__ G, int n, const aos2_triang_obs_t *__restrict__ obs1,
                                                              const aos2_triang_obs_t *__restrict__ obs2, float *__restrict__ x3D_out,
                                                              uint8_t *__restrict__ status_out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    const TriKf K1 = {G->Tcw1, G->fx1, G->fy1, G->cx1, G->cy1, G->mb1, G->mbf1, G->scale_factors1};
    const TriKf K2 = {G->Tcw2, G->fx2, G->fy2, G->cx2, G->cy2, G->mb2, G->mbf2, G->scale_factors2};
    TriObs q1 = {}, q2 = {};
    if (k < n) {
        const aos2_triang_obs_t a = obs1[k], b = obs2[k];
        q1 = TriObs{a.ux, a.uy, a.kx, a.ky, a.u_right, a.depth, a.octave};
        q2 = TriObs{b.ux, b.uy, b.kx, b.ky, b.u_right, b.depth, b.octave};
    }
    float x3D[3];
    const int st = tri_block(k < n, K1, K2, q1, q2, x3D);
    if (k < n) {
        status_out[k] = (uint8_t)st;
        x3D_out[3 * (size_t)k] = x3D[0]; x3D_out[3 * (size_t)k + 1] = x3D[1]; x3D_out[3 * (size_t)k + 2] = x3D[2];
    }
}

// the argument checks of aos2_triangulate_matches and of the host tap: everything triangulate_pair indexes with
int triang_check(const aos2_triang_geom_t *g, int n, const aos2_triang_obs_t *obs1, const aos2_triang_obs_t *obs2, const float *x3D,
                 const uint8_t *status)
{
    if (!g || n < 0 || (n > 0 && (!obs1 || !obs2 || !x3D || !status)) || g->n_levels < 2 || g->n_levels > 8) {
        set_error("bad argument (geometry, per-match arrays, 2..8 pyramid levels)");
        return AOS2_ERR_ARG;
    }
    for (int k = 0; k < n; ++k)
        if (obs1[k].octave < 0 || obs1[k].octave >= g->n_levels || obs2[k].octave < 0 || obs2[k].octave >= g->n_levels) {
            set_error("match %d: octaves (%d, %d) outside the %d pyramid levels", k, obs1[k].octave, obs2[k].octave, g->n_levels);
            return AOS2_ERR_ARG;
        }
    return AOS2_OK;
}

}  // namespace aos2

extern "C" {

int aos2_triangulate_matches(aos2_matcher_t *m, const aos2_triang_geom_t *g, int n, const aos2_triang_obs_t *obs1,
                             const aos2_triang_obs_t *obs2, float *x3D, uint8_t *status)
{
    using namespace aos2;
    if (!m) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = triang_check(g, n, obs1, obs2, x3D, status);
    if (st || n == 0) return st;
    if ((st = matcher_init(m))) return st;
    Arena A{m};
    const aos2_triang_geom_t *d_g;
    const aos2_triang_obs_t *d_o1, *d_o2;
    float *d_x;
    uint8_t *d_s;
    A.in(d_g, g, sizeof(*g));
    A.in(d_o1, obs1, sizeof(aos2_triang_obs_t) * (size_t)n);
    A.in(d_o2, obs2, sizeof(aos2_triang_obs_t) * (size_t)n);
    A.out(d_x, 12 * (size_t)n);
    A.out(d_s, (size_t)n);
    if ((st = A.upload())) return st;
    if ((st = A.begin())) return st;
    hipLaunchKernelGGL(triangulate_list_kernel, dim3((n + 255) / 256), dim3(256), 0, m->stream, d_g, n, d_o1, d_o2, d_x, d_s);
    A.fetch(x3D, d_x, 12 * (size_t)n);
    A.fetch(status, d_s, (size_t)n);
    return A.end();
}

}  // extern "C"
