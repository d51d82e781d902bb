// Optimizer::OptimizeEssentialGraph on gfx950 for a batch of pose graphs (include/aos2.h: aos2_optimize_essential_graph; reference
// src/Optimizer.cc:782-1045).  The arithmetic is csrc/essential_graph.h, shared with the host tap at the end of this file.
//
// The pattern of H does not change over the iterations, so the host works it out once per problem (eg_symbolic): the 7x7 block
// pattern over the free vertices in ascending vertex order, the pattern of L by the elimination tree, for every block the list of
// edges that add to it (in edge order), and for every column of L the blocks its trailing update lands in.  The values never
// leave the device: an LM iteration is k_eg_perturb, k_eg_linearise, k_eg_assemble, k_eg_begin and up to ten (k_eg_factor_solve,
// k_eg_trial) pairs, each of which returns at once when the iteration's trials are over; rho, lambda, ni and which estimates stay
// are decided in k_eg_trial.  The host reads the control words once per iteration to stop enqueueing.
#include <algorithm>
#include <vector>

#include "block_ldlt.h"
#include "essential_graph.h"

namespace aos2 {

constexpr int kEgThreads = 256, kEgRows = kEgThreads / 16;
constexpr int kEgMaxVertices = 8192, kEgMaxProblems = 16, kEgHostMaxVertices = 512;
constexpr size_t kEgArenaMax = (size_t)2 << 30;

// (A + lambda I) x = b in 7x7 blocks, block_ldlt.h
using EgSystem = BlockSystem;
static_assert(kEgThreads == kBlockLdltThreads, "k_eg_factor_solve is one workgroup of block_factor_solve");

struct EgDev {
    int32_t nv, ne, np, fixed, fix_scale, pad;
    const int32_t *v0, *v1;
    const Sim3d *C, *S_in;            // the measurements [ne], vScw [nv]
    Sim3d *est, *est_try, *pert;      // [nv], [nv], [nv][kEgPert]
    double *J, *E;                    // [ne][2][49], [ne][7]
    const int32_t *hidx, *free_v;     // [nv] hessian index or -1, [nf] its inverse
    const int32_t *slot_ptr, *slot_list;   // [n_slots + 1], entries edge * 4 + kind (eg_block_term)
    const int32_t *b_ptr, *b_list;         // [nf + 1], entries edge * 2 + side
    EgSystem sys;
    EgControl *ctl;
    const float *Xw_in;
    const int32_t *ref;
    float *Tiw, *Xw_out;
};

// the transforms of a linearisation that belong to a vertex: grid over (vertex, 15): the 14 perturbed estimates with their inverses,
// and the inverse of the estimate
__global__ __launch_bounds__(kEgThreads) void k_eg_perturb(const EgDev *__restrict__ probs)
{
    const EgDev &P = probs[blockIdx.y];
    if (!P.ctl->running) return;
    const int item = blockIdx.x * kEgThreads + threadIdx.x;
    if (item >= P.nv * 15) return;
    const int v = item / 15, k = item % 15;
    const Sim3d S = P.est[v];
    Sim3d *out = P.pert + (size_t)v * kEgPert;
    if (k == 14) {
        Sim3d inv;
        so_inverse(S, inv);
        out[0] = inv;
    } else if (P.hidx[v] >= 0) {   // (a fixed vertex is never perturbed)
        Sim3d fwd, inv;
        so_perturbed(S, k, P.fix_scale != 0, fwd, inv);
        out[1 + 2 * k] = fwd;
        out[2 + 2 * k] = inv;
    }
}

// grid over (edge, 16): items 0..13 = column d of the Jacobian of side 0 / side 1 (two residuals each), item 14 = the stored residual
__global__ __launch_bounds__(kEgThreads) void k_eg_linearise(const EgDev *__restrict__ probs)
{
    const EgDev &P = probs[blockIdx.y];
    if (!P.ctl->running) return;
    const int item = blockIdx.x * kEgThreads + threadIdx.x;
    if (item >= P.ne * 16) return;
    const int e = item >> 4, j = item & 15;
    if (j == 15) return;
    const int a = P.v0[e], b = P.v1[e];
    const Sim3d C = P.C[e];
    const Sim3d *pa = P.pert + (size_t)a * kEgPert, *pb = P.pert + (size_t)b * kEgPert;
    if (j == 14) {
        double er[7];
        eg_residual(C, P.est[a], pb[0], er);
        for (int r = 0; r < 7; ++r) P.E[(size_t)e * 7 + r] = er[r];
        return;
    }
    const int side = j / 7, d = j % 7;
    if (P.hidx[side ? b : a] < 0) return;   // the Jacobian of a fixed vertex is never read
    eg_jacobian_column(C, P.est[a], pa, pb, side, d, P.J + ((size_t)e * 2 + side) * 49);
}

// grid over the entries of the blocks of H and the components of b: each is summed over its list of edges, in edge order
__global__ __launch_bounds__(kEgThreads) void k_eg_assemble(const EgDev *__restrict__ probs)
{
    const EgDev &P = probs[blockIdx.y];
    if (!P.ctl->running) return;
    const long long item = (long long)blockIdx.x * kEgThreads + threadIdx.x, nH = (long long)P.sys.n_slots * 49;
    if (item < nH) {
        const int slot = (int)(item / 49), ent = (int)(item % 49), a = ent / 7, b = ent % 7;
        double s = 0;
        for (int q = P.slot_ptr[slot]; q < P.slot_ptr[slot + 1]; ++q) {
            const int w = P.slot_list[q];
            s += eg_block_term(P.J + (size_t)(w >> 2) * 98, w & 3, a, b);
        }
        const_cast<double *>(P.sys.H)[item] = s;
    } else if (item < nH + (long long)P.sys.nf * 7) {
        const int i = (int)(item - nH), h = i / 7, a = i % 7;
        double s = 0;
        for (int q = P.b_ptr[h]; q < P.b_ptr[h + 1]; ++q) {
            const int w = P.b_list[q];
            s -= eg_jte(P.J + (size_t)w * 49, P.E + (size_t)(w >> 1) * 7, a);
        }
        const_cast<double *>(P.sys.b)[i] = s;
    }
}

// chi2 of the stored residuals, edge e in thread e % 256, and the start of the iteration; one workgroup per problem
__global__ __launch_bounds__(kEgThreads) void k_eg_begin(const EgDev *__restrict__ probs)
{
    __shared__ double part[kEgRows];
    const EgDev &P = probs[blockIdx.x];
    if (!P.ctl->running) return;
    double chi[1] = {0};
    for (int e = threadIdx.x; e < P.ne; e += kEgThreads) chi[0] += eg_chi2(P.E + (size_t)e * 7);
    block_sum_f64(chi, part);
    if (threadIdx.x == 0) eg_iteration_begin(*P.ctl, chi[0]);
}

// Block-sparse LDL^T of H + lambda I in device memory and the solve, one workgroup per system: block_ldlt.h with 7x7 blocks
__device__ __forceinline__ void eg_factor_solve(const EgSystem &S, double lambda, int32_t *solved) { block_factor_solve<7>(S, lambda, solved); }

__global__ __launch_bounds__(kEgThreads) void k_eg_factor_solve(const EgDev *__restrict__ probs)
{
    const EgDev &P = probs[blockIdx.x];
    EgControl *ctl = P.ctl;
    if (!ctl->running || !ctl->open) return;
    eg_factor_solve(P.sys, ctl->lm.lambda, &ctl->solved);
}

// the same on a system alone (aos2_debug_essential_graph_solve_device)
__global__ __launch_bounds__(kEgThreads) void k_eg_factor_solve_tap(EgSystem S, double lambda, int32_t *solved) { eg_factor_solve(S, lambda, solved); }

// One trial, one workgroup per problem: the estimates of the free vertices after oplus(x) into est_try, the residuals and chi2 (edge e
// in thread e % 256), the decision; est_try becomes est when the trial is accepted.  kTap: the two sums the decision is taken on go to
// tap[0], tap[1] as well (aos2_debug_essential_graph_trial_device).
template <bool kTap>
__device__ __forceinline__ void eg_trial(const EgDev &P, double *tap)
{
    __shared__ double part[kEgRows * 2];
    __shared__ int accepted;
    EgControl *ctl = P.ctl;
    if (!ctl->running || !ctl->open) return;
    const int tid = threadIdx.x, nf = P.sys.nf;
    const double lambda = ctl->lm.lambda;
    double sum[2] = {0, 0};   // chi2, sum of x (lambda x + b)
    for (int h = tid; h < nf; h += kEgThreads) {
        double u[7];
        for (int r = 0; r < 7; ++r) u[r] = P.sys.x[7 * h + r];
        const int v = P.free_v[h];
        Sim3d T;
        so_oplus(u, P.fix_scale != 0, P.est[v], T);
        P.est_try[v] = T;
    }
    for (int i = tid; i < 7 * nf; i += kEgThreads) {
        const double x = P.sys.x[i];
        sum[1] += x * (lambda * x + P.sys.b[i]);
    }
    __syncthreads();
    for (int e = tid; e < P.ne; e += kEgThreads) {
        Sim3d inv;
        so_inverse(P.est_try[P.v1[e]], inv);
        double er[7];
        eg_residual(P.C[e], P.est_try[P.v0[e]], inv, er);
        sum[0] += eg_chi2(er);
    }
    block_sum_f64(sum, part);
    if (kTap && tid == 0) {
        tap[0] = sum[0];
        tap[1] = sum[1];
    }
    if (tid == 0) accepted = eg_trial_decide(*ctl, sum[0], sum[1]);
    __syncthreads();
    if (accepted)
        for (int h = tid; h < nf; h += kEgThreads) {
            const int v = P.free_v[h];
            P.est[v] = P.est_try[v];
        }
}

__global__ __launch_bounds__(kEgThreads) void k_eg_trial(const EgDev *__restrict__ probs) { eg_trial<false>(probs[blockIdx.x], nullptr); }

// the same on one problem, with the sums (aos2_debug_essential_graph_trial_device)
__global__ __launch_bounds__(kEgThreads) void k_eg_trial_tap(const EgDev *__restrict__ probs, double *tap) { eg_trial<true>(probs[0], tap); }

// grid over max(vertices, points): the SE3 pose of a vertex, the corrected position of a point
__global__ __launch_bounds__(kEgThreads) void k_eg_finish(const EgDev *__restrict__ probs)
{
    const EgDev &P = probs[blockIdx.y];
    const int item = blockIdx.x * kEgThreads + threadIdx.x;
    if (item < P.nv) eg_pose(P.est[item], P.Tiw + (size_t)item * 16);
    if (item < P.np) {
        const int r = P.ref[item];
        eg_point(P.S_in[r], P.est[r], P.Xw_in + (size_t)item * 3, P.Xw_out + (size_t)item * 3);
    }
}

// ---------------------------------------------------------------------------------------------- the symbolic phase (host)
using EgSymbolic = BlockSymbolic;
static bool eg_symbolic(int nf, const std::vector<int32_t> &hi, const std::vector<int32_t> &lo, size_t max_bytes, EgSymbolic &Y)
{
    return block_symbolic(nf, hi, lo, 49, max_bytes, Y);
}

// one problem as the host sees it: the hessian indices, the lower-triangle pairs of its edges, the lists of the assembly
struct EgHostGraph {
    int nf = 0;
    bool runs = false;   // LM has something to do
    std::vector<int32_t> hidx, free_v, hi, lo;
    EgSymbolic Y;
    std::vector<int32_t> slot_ptr, slot_list, b_ptr, b_list;
};

static void eg_indices(const aos2_essential_graph_problem_t &P, EgHostGraph &G)
{
    G.hidx.assign((size_t)P.n_vertices, -1);
    G.free_v.clear();
    for (int v = 0; v < P.n_vertices; ++v)
        if (v != P.fixed) {
            G.hidx[(size_t)v] = (int32_t)G.free_v.size();
            G.free_v.push_back(v);
        }
    G.nf = (int)G.free_v.size();
    G.runs = G.nf > 0 && P.n_edges > 0;
    G.hi.clear();
    G.lo.clear();
    for (int e = 0; e < P.n_edges; ++e) {
        const int a = G.hidx[(size_t)P.v0[e]], b = G.hidx[(size_t)P.v1[e]];
        if (a >= 0 && b >= 0) {
            G.hi.push_back(std::max(a, b));
            G.lo.push_back(std::min(a, b));
        }
    }
}

// the edge lists of every slot of H and of every segment of b, in edge order (a counting sort by slot keeps it)
static void eg_lists(const aos2_essential_graph_problem_t &P, EgHostGraph &G)
{
    const size_t n_slots = (size_t)G.nf + G.Y.l_blocks();
    std::vector<int32_t> where, what, bwhere, bwhat;
    for (int e = 0; e < P.n_edges; ++e) {
        const int a = G.hidx[(size_t)P.v0[e]], b = G.hidx[(size_t)P.v1[e]];
        if (a >= 0) {
            where.push_back(a); what.push_back(e * 4);
            bwhere.push_back(a); bwhat.push_back(e * 2);
        }
        if (b >= 0) {
            where.push_back(b); what.push_back(e * 4 + 1);
            bwhere.push_back(b); bwhat.push_back(e * 2 + 1);
        }
        if (a >= 0 && b >= 0) {
            where.push_back(G.Y.slot(std::max(a, b), std::min(a, b)));
            what.push_back(e * 4 + (a > b ? 2 : 3));
        }
    }
    auto bucket = [](const std::vector<int32_t> &wh, const std::vector<int32_t> &wt, size_t n, std::vector<int32_t> &ptr, std::vector<int32_t> &list) {
        ptr.assign(n + 1, 0);
        for (int32_t w : wh) ptr[(size_t)w + 1]++;
        for (size_t i = 0; i < n; ++i) ptr[i + 1] += ptr[i];
        list.assign(wh.size(), 0);
        std::vector<int32_t> at(ptr.begin(), ptr.end() - 1);
        for (size_t i = 0; i < wh.size(); ++i) list[(size_t)at[(size_t)wh[i]]++] = wt[i];
    };
    bucket(where, what, n_slots, G.slot_ptr, G.slot_list);
    bucket(bwhere, bwhat, (size_t)G.nf, G.b_ptr, G.b_list);
}

static int eg_check(const aos2_essential_graph_problem_t *p, const aos2_essential_graph_result_t *r, int n_problems, int max_vertices)
{
    if (n_problems < 0 || n_problems > kEgMaxProblems || (n_problems > 0 && (!p || !r))) {
        set_error("bad argument (0..%d problems and their results)", kEgMaxProblems);
        return AOS2_ERR_ARG;
    }
    for (int i = 0; i < n_problems; ++i) {
        const aos2_essential_graph_problem_t &P = p[i];
        bool ok = P.n_vertices >= 1 && P.n_edges >= 0 && P.n_points >= 0 && P.iterations >= 1 && P.Scw && r[i].Scw && r[i].Tiw &&
                  P.fixed >= 0 && P.fixed < P.n_vertices && (P.n_edges == 0 || (P.v0 && P.v1 && P.Sji)) &&
                  (P.n_points == 0 || (P.Xw && P.ref && r[i].Xw));
        for (int e = 0; ok && e < P.n_edges; ++e)
            ok = P.v0[e] >= 0 && P.v0[e] < P.n_vertices && P.v1[e] >= 0 && P.v1[e] < P.n_vertices && P.v0[e] != P.v1[e];
        for (int k = 0; ok && k < P.n_points; ++k) ok = P.ref[k] >= 0 && P.ref[k] < P.n_vertices;
        if (!ok) {
            set_error("problem %d: bad argument (counts >= 0, n_vertices >= 1, iterations >= 1, the arrays, fixed / v0 / v1 / ref in range, v0 != v1)", i);
            return AOS2_ERR_ARG;
        }
    }
    for (int i = 0; i < n_problems; ++i)
        if (p[i].n_vertices > max_vertices || p[i].n_edges > (1 << 26)) {
            set_error("problem %d: more than %d vertices or 2^26 edges", i, max_vertices);
            return AOS2_ERR_CAPACITY;
        }
    return AOS2_OK;
}

static void eg_result_control(const EgControl &c, bool ran, int l_blocks, aos2_essential_graph_result_t &R)
{
    R.chi2_initial = ran ? c.chi2_initial : 0;
    R.chi2_final = ran ? c.lm.currentChi : 0;
    R.iterations = c.iterations;
    R.trials = c.trials;
    R.rejected = c.rejected;
    R.l_blocks = l_blocks;
    R.status = ran && c.accepted_first == 0 ? AOS2_EG_NO_STEP : AOS2_EG_OK;
}

// the symbolic phase of a batch inside the memory a call may take: the indices, the pattern of L and the lists of every problem
static int eg_host_phase(const aos2_essential_graph_problem_t *p, int n, std::vector<EgHostGraph> &G)
{
    size_t budget = kEgArenaMax;
    for (int i = 0; i < n; ++i) {
        const aos2_essential_graph_problem_t &P = p[i];
        EgHostGraph &g = G[(size_t)i];
        eg_indices(P, g);
        const size_t fixed_bytes = (size_t)P.n_vertices * (sizeof(Sim3d) * (3 + kEgPert) + 64 + 8) + (size_t)P.n_edges * (98 * 8 + 56 + 64 + 8 + 40) +
                                   (size_t)P.n_points * 28 + 64 * 256;
        if (fixed_bytes > budget || (g.runs && !eg_symbolic(g.nf, g.hi, g.lo, budget - fixed_bytes, g.Y))) {
            set_error("problem %d: the graph and its factor do not fit the %zu MiB a call may take", i, kEgArenaMax >> 20);
            return AOS2_ERR_EG_MEMORY;
        }
        if (!g.runs) {
            g.Y = EgSymbolic();
            g.Y.nf = g.nf;
            g.Y.colptr.assign((size_t)g.nf + 1, 0);
            g.Y.upd_ptr.assign((size_t)g.nf + 1, 0);
        }
        const size_t taken = fixed_bytes + (g.Y.l_blocks() + (size_t)g.nf) * 49 * 8 * 2 + g.Y.upd_dst.size() * 4;
        if (taken > budget) {   // (a problem without LM keeps its diagonal blocks too)
            set_error("problem %d: the batch does not fit the %zu MiB a call may take", i, kEgArenaMax >> 20);
            return AOS2_ERR_EG_MEMORY;
        }
        budget -= taken;
        eg_lists(P, g);
    }
    return AOS2_OK;
}

static const Sim3d *eg_sim3(const double *p) { return reinterpret_cast<const Sim3d *>(p); }

// The layout of a call: what the host stages (a prefix of the arena: per problem the graph and its lists, the EgDev table, the
// control words, the estimates), what comes back (neighbours, read together: the control words first, read once per iteration, then
// per problem Scw, Tiw, Xw) and the scratch.  Every array is registered with the field of the table that points at it (regions.h),
// so the object stays where it is between plan() and bind().  The call and the taps share it.
struct EgLayout {
    HostArena H;
    std::vector<EgDev> dev;          // the table as bind() completes it
    const EgDev *dprobs = nullptr;   // ... and where the kernels find it
    EgControl *ctl = nullptr;        // [n]: the start of what comes back
    size_t o_probs = 0, in_bytes = 0, res_bytes = 0;
    long long max_v = 1, max_e = 1, max_asm = 1, max_fin = 1;   // the largest grids of the batch: vertices, edges, entries of H and b, finish items

    void plan(const aos2_essential_graph_problem_t *p, int n, const std::vector<EgHostGraph> &G)
    {
        dev.resize((size_t)n);
        memset((void *)dev.data(), 0, sizeof(EgDev) * (size_t)n);
        std::vector<EgControl> ctl0((size_t)n);
        for (int i = 0; i < n; ++i) {
            const aos2_essential_graph_problem_t &P = p[i];
            const EgHostGraph &g = G[(size_t)i];
            EgDev &D = dev[(size_t)i];
            const size_t nv = (size_t)P.n_vertices, ne = (size_t)P.n_edges, np = (size_t)P.n_points;
            D.nv = P.n_vertices; D.ne = P.n_edges; D.np = P.n_points; D.fixed = P.fixed; D.fix_scale = P.fix_scale != 0;
            D.sys.nf = g.nf; D.sys.n_slots = g.nf + (int32_t)g.Y.l_blocks();
            H.in(D.v0, P.v0, ne);
            H.in(D.v1, P.v1, ne);
            H.in(D.C, eg_sim3(P.Sji), ne);
            H.in(D.S_in, eg_sim3(P.Scw), nv);
            H.in(D.est_try, eg_sim3(P.Scw), nv);
            H.in(D.hidx, g.hidx);
            H.in(D.free_v, g.free_v);
            H.in(D.slot_ptr, g.slot_ptr);
            H.in(D.slot_list, g.slot_list);
            H.in(D.b_ptr, g.b_ptr);
            H.in(D.b_list, g.b_list);
            H.in(D.sys.colptr, g.Y.colptr);
            H.in(D.sys.rowidx, g.Y.rowidx);
            H.in(D.sys.upd_ptr, g.Y.upd_ptr);
            H.in(D.sys.upd_dst, g.Y.upd_dst);
            H.in(D.Xw_in, P.Xw, 3 * np);
            H.in(D.ref, P.ref, np);
            eg_control_init(ctl0[(size_t)i], P.iterations, g.runs);
            max_v = std::max<long long>(max_v, P.n_vertices);
            max_e = std::max<long long>(max_e, P.n_edges);
            max_asm = std::max<long long>(max_asm, ((long long)g.nf + (long long)g.Y.l_blocks()) * 49 + 7LL * g.nf);
            max_fin = std::max<long long>(max_fin, std::max(P.n_vertices, P.n_points));
        }
        o_probs = H.in(dprobs, dev.data(), (size_t)n);   // (bind() writes the table there)
        // The estimates and the control words are staged (inputs), the rest is scratch.
        const size_t o_ctl = H.in(ctl, ctl0.data(), (size_t)n);
        for (int i = 0; i < n; ++i) H.at(dev[(size_t)i].ctl, o_ctl + sizeof(EgControl) * (size_t)i);
        for (int i = 0; i < n; ++i) H.in(dev[(size_t)i].est, eg_sim3(p[i].Scw), (size_t)p[i].n_vertices);
        in_bytes = H.host_size;
        for (int i = 0; i < n; ++i) {
            H.room(dev[(size_t)i].Tiw, 16 * (size_t)p[i].n_vertices);
            H.room(dev[(size_t)i].Xw_out, 3 * (size_t)p[i].n_points);
        }
        res_bytes = H.size - o_ctl;
        for (int i = 0; i < n; ++i) {
            EgDev &D = dev[(size_t)i];
            const size_t nv = (size_t)D.nv, ne = (size_t)D.ne, n_slots = (size_t)D.sys.n_slots, nx = 7 * (size_t)D.sys.nf;
            H.room(D.pert, kEgPert * nv);
            H.room(D.J, 98 * ne);
            H.room(D.E, 7 * ne);
            H.room(D.sys.H, 49 * n_slots);
            H.room(D.sys.L, 49 * n_slots);
            H.room(D.sys.b, nx);
            H.room(D.sys.y, nx);
            H.room(D.sys.x, nx);
        }
    }

    // points the table at the arena at `base` and writes it into the staged prefix -> where the kernels find it
    const EgDev *bind(uint8_t *base)
    {
        H.bind(base);
        memcpy(H.own.data() + o_probs, dev.data(), sizeof(EgDev) * dev.size());
        return dprobs;
    }
};

// ---------------------------------------------------------------------------------------------- the host tap
static void eg_host_one(const aos2_essential_graph_problem_t &P, EgHostGraph &G, aos2_essential_graph_result_t &R)
{
    const int nv = P.n_vertices, ne = P.n_edges;
    std::vector<Sim3d> est(eg_sim3(P.Scw), eg_sim3(P.Scw) + nv), trial_est;
    const Sim3d *C = eg_sim3(P.Sji);
    EgControl ctl;
    eg_control_init(ctl, P.iterations, G.runs);
    if (G.runs) {
        SkylineLdlt K;
        K.shape(G.nf, G.hi, G.lo, 7);
        std::vector<Sim3d> pert((size_t)nv * kEgPert);
        std::vector<double> J((size_t)ne * 98), E((size_t)ne * 7), b((size_t)K.n), x((size_t)K.n, 0.0);
        const bool fix = P.fix_scale != 0;
        while (ctl.running) {
            for (int v = 0; v < nv; ++v) {
                Sim3d *o = pert.data() + (size_t)v * kEgPert;
                so_inverse(est[(size_t)v], o[0]);
                if (G.hidx[(size_t)v] >= 0)
                    for (int k = 0; k < 14; ++k) so_perturbed(est[(size_t)v], k, fix, o[1 + 2 * k], o[2 + 2 * k]);
            }
            std::fill(K.A.begin(), K.A.end(), 0.0);
            std::fill(b.begin(), b.end(), 0.0);
            double chi = 0;
            for (int e = 0; e < ne; ++e) {
                const int va = P.v0[e], vb = P.v1[e], h[2] = {G.hidx[(size_t)va], G.hidx[(size_t)vb]};
                const Sim3d *pa = pert.data() + (size_t)va * kEgPert, *pb = pert.data() + (size_t)vb * kEgPert;
                double *Je = J.data() + (size_t)e * 98, *Ee = E.data() + (size_t)e * 7;
                eg_residual(C[e], est[(size_t)va], pb[0], Ee);
                chi += eg_chi2(Ee);
                for (int side = 0; side < 2; ++side)
                    if (h[side] >= 0)
                        for (int d = 0; d < 7; ++d) eg_jacobian_column(C[e], est[(size_t)va], pa, pb, side, d, Je + side * 49);
                for (int side = 0; side < 2; ++side) {
                    if (h[side] < 0) continue;
                    for (int r = 0; r < 7; ++r) {
                        for (int c = 0; c <= r; ++c) K.a(K.A, 7 * h[side] + r, 7 * h[side] + c) += eg_block_term(Je, side, r, c);
                        b[(size_t)(7 * h[side] + r)] -= eg_jte(Je + side * 49, Ee, r);
                    }
                }
                if (h[0] >= 0 && h[1] >= 0) {
                    const int hi = std::max(h[0], h[1]), lo = std::min(h[0], h[1]), kind = h[0] > h[1] ? 2 : 3;
                    for (int r = 0; r < 7; ++r)
                        for (int c = 0; c < 7; ++c) K.a(K.A, 7 * hi + r, 7 * lo + c) += eg_block_term(Je, kind, r, c);
                }
            }
            eg_iteration_begin(ctl, chi);
            while (ctl.open) {
                ctl.solved = K.solve(ctl.lm.lambda, b, x);
                trial_est = est;
                for (int hf = 0; hf < G.nf; ++hf) {
                    double u[7];
                    for (int r = 0; r < 7; ++r) u[r] = x[(size_t)(7 * hf + r)];
                    const int v = G.free_v[(size_t)hf];
                    so_oplus(u, fix, est[(size_t)v], trial_est[(size_t)v]);
                }
                double scale = 0, temp = 0;
                for (int i = 0; i < K.n; ++i) scale += x[(size_t)i] * (ctl.lm.lambda * x[(size_t)i] + b[(size_t)i]);
                for (int e = 0; e < ne; ++e) {
                    Sim3d inv;
                    so_inverse(trial_est[(size_t)P.v1[e]], inv);
                    double er[7];
                    eg_residual(C[e], trial_est[(size_t)P.v0[e]], inv, er);
                    temp += eg_chi2(er);
                }
                if (eg_trial_decide(ctl, temp, scale)) est = trial_est;
            }
        }
    }
    eg_result_control(ctl, G.runs, (int)G.Y.l_blocks(), R);
    memcpy(R.Scw, est.data(), sizeof(Sim3d) * (size_t)nv);
    for (int v = 0; v < nv; ++v) eg_pose(est[(size_t)v], R.Tiw + (size_t)v * 16);
    for (int k = 0; k < P.n_points; ++k) eg_point(eg_sim3(P.Scw)[P.ref[k]], est[(size_t)P.ref[k]], P.Xw + (size_t)k * 3, R.Xw + (size_t)k * 3);
}

static inline int eg_blocks(long long items) { return (int)std::max<long long>(1, (items + kEgThreads - 1) / kEgThreads); }

// ---------------------------------------------------------------------------------------------- the device taps
// One problem through the call's own host phase and layout, and its first linearisation (k_eg_perturb, k_eg_linearise, k_eg_assemble,
// k_eg_begin with running = 1) enqueued on the handle's stream.  J is pre-filled with the byte 0x5A: what no kernel writes keeps it.
struct EgTap {
    std::vector<EgHostGraph> G;
    EgLayout Lay;
    double *sums = nullptr;   // the two doubles of k_eg_trial_tap
};

static int eg_tap_linearise(aos2_lba_t *s, const aos2_essential_graph_problem_t *p, EgTap &T)
{
    aos2_essential_graph_result_t none;
    memset(&none, 0, sizeof none);
    double dummy_d = 0;
    float dummy_f = 0;
    none.Scw = &dummy_d;   // (eg_check wants a result; the taps write none)
    none.Tiw = none.Xw = &dummy_f;
    if (!s || !p) {
        set_error("bad argument (the handle, the problem)");
        return AOS2_ERR_ARG;
    }
    int st = eg_check(p, &none, 1, kEgHostMaxVertices);
    if (st) return st;
    T.G.resize(1);
    if ((st = eg_host_phase(p, 1, T.G))) return st;
    if (!T.G[0].runs) {
        set_error("bad argument (a problem with a free vertex and an edge)");
        return AOS2_ERR_ARG;
    }
    T.Lay.plan(p, 1, T.G);
    T.Lay.H.room(T.sums, 2);
    if ((st = lba_handle_init(s))) return st;
    if ((st = s->arena.alloc(T.Lay.H.size + 256))) return st;
    const EgDev *dprobs = T.Lay.bind(s->arena.p);
    const EgDev &D = T.Lay.dev[0];
    hipStream_t q = s->stream;
    AOS2_HIP_CHECK(hipMemcpyAsync(s->arena.p, T.Lay.H.data(), T.Lay.in_bytes, hipMemcpyHostToDevice, q));
    AOS2_HIP_CHECK(hipMemsetAsync(D.sys.x, 0, bytes_of(D.sys.x, 7 * (size_t)D.sys.nf), q));
    AOS2_HIP_CHECK(hipMemsetAsync(D.J, 0x5A, bytes_of(D.J, 98 * (size_t)D.ne), q));
    hipLaunchKernelGGL(k_eg_perturb, dim3(eg_blocks(T.Lay.max_v * 15), 1), dim3(kEgThreads), 0, q, dprobs);
    hipLaunchKernelGGL(k_eg_linearise, dim3(eg_blocks(T.Lay.max_e * 16), 1), dim3(kEgThreads), 0, q, dprobs);
    hipLaunchKernelGGL(k_eg_assemble, dim3(eg_blocks(T.Lay.max_asm), 1), dim3(kEgThreads), 0, q, dprobs);
    hipLaunchKernelGGL(k_eg_begin, dim3(1), dim3(kEgThreads), 0, q, dprobs);
    return AOS2_OK;
}

}  // namespace aos2

using namespace aos2;
static_assert(sizeof(Sim3d) == 64, "a Sim3 is the 8 doubles of the C ABI");

extern "C" {

int aos2_optimize_essential_graph(aos2_lba_t *s, const aos2_essential_graph_problem_t *p, aos2_essential_graph_result_t *r, int n_problems)
{
    if (!s) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = eg_check(p, r, n_problems, kEgMaxVertices);
    if (st || n_problems == 0) return st;
    const int n = n_problems;
    // the symbolic phase, and everything the device reads, as one staged prefix of the arena
    std::vector<EgHostGraph> G((size_t)n);
    if ((st = eg_host_phase(p, n, G))) return st;
    EgLayout Lay;
    Lay.plan(p, n, G);
    if (Lay.H.size + 256 > kEgArenaMax + ((size_t)64 << 20)) {
        set_error("the batch does not fit the %zu MiB a call may take", kEgArenaMax >> 20);
        return AOS2_ERR_EG_MEMORY;
    }
    if ((st = lba_handle_init(s))) return st;
    s->last_essential_graph_ms = 0;
    if ((st = s->arena.alloc(Lay.H.size + 256))) return st;
    if ((st = s->h_stage.alloc(Lay.res_bytes + 64))) return st;
    uint8_t *base = s->arena.p;
    const EgDev *dprobs = Lay.bind(base);
    const std::vector<EgDev> &dev = Lay.dev;
    const size_t res_bytes = Lay.res_bytes;
    const long long max_v = Lay.max_v, max_e = Lay.max_e, max_asm = Lay.max_asm, max_fin = Lay.max_fin;
    bool any = false;
    for (int i = 0; i < n; ++i) any = any || G[(size_t)i].runs;
    hipStream_t q = s->stream;
    AOS2_HIP_CHECK(hipMemcpyAsync(base, Lay.H.data(), Lay.in_bytes, hipMemcpyHostToDevice, q));
    AOS2_HIP_CHECK(hipEventRecord(s->ev[0], q));
    // x starts at zero: a first solve that fails applies the solver's vector as it stands
    for (int i = 0; i < n; ++i)
        if (G[(size_t)i].nf > 0) AOS2_HIP_CHECK(hipMemsetAsync(dev[(size_t)i].sys.x, 0, bytes_of(dev[(size_t)i].sys.x, 7 * (size_t)G[(size_t)i].nf), q));
    EgControl *hctl = (EgControl *)s->h_stage.p;
    int max_it = 0;
    for (int i = 0; i < n; ++i)
        if (G[(size_t)i].runs) max_it = std::max(max_it, (int)p[i].iterations);
    // profiling (aos2_debug_essential_graph_profile): an event pair around every launch, summed per family after the call
    LaunchProfiler prof{s->eg_profile, q};
    for (int it = 0; any && it < max_it; ++it) {
        prof.mark(0, true);
        hipLaunchKernelGGL(k_eg_perturb, dim3(eg_blocks(max_v * 15), n), dim3(kEgThreads), 0, q, dprobs);
        hipLaunchKernelGGL(k_eg_linearise, dim3(eg_blocks(max_e * 16), n), dim3(kEgThreads), 0, q, dprobs);
        prof.mark(0, false);
        prof.mark(1, true);
        hipLaunchKernelGGL(k_eg_assemble, dim3(eg_blocks(max_asm), n), dim3(kEgThreads), 0, q, dprobs);
        prof.mark(1, false);
        prof.mark(3, true);
        hipLaunchKernelGGL(k_eg_begin, dim3(n), dim3(kEgThreads), 0, q, dprobs);
        prof.mark(3, false);
        for (int t = 0; t < 10; ++t) {
            prof.mark(2, true);
            hipLaunchKernelGGL(k_eg_factor_solve, dim3(n), dim3(kEgThreads), 0, q, dprobs);
            prof.mark(2, false);
            prof.mark(3, true);
            hipLaunchKernelGGL(k_eg_trial, dim3(n), dim3(kEgThreads), 0, q, dprobs);
            prof.mark(3, false);
        }
        AOS2_HIP_CHECK(hipMemcpyAsync(hctl, Lay.ctl, sizeof(EgControl) * (size_t)n, hipMemcpyDeviceToHost, q));
        AOS2_HIP_CHECK(hipStreamSynchronize(q));
        AOS2_HIP_CHECK(hipGetLastError());
        any = false;
        for (int i = 0; i < n; ++i) any = any || hctl[i].running;
    }
    prof.mark(4, true);
    hipLaunchKernelGGL(k_eg_finish, dim3(eg_blocks(max_fin), n), dim3(kEgThreads), 0, q, dprobs);
    prof.mark(4, false);
    AOS2_HIP_CHECK(hipEventRecord(s->ev[1], q));
    AOS2_HIP_CHECK(hipMemcpyAsync(s->h_stage.p, Lay.ctl, res_bytes, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    AOS2_HIP_CHECK(hipGetLastError());
    (void)hipEventElapsedTime(&s->last_essential_graph_ms, s->ev[0], s->ev[1]);
    prof.sum(s->eg_family_ms, 5);
    const uint8_t *res = s->h_stage.p;
    for (int i = 0; i < n; ++i) {
        const EgDev &D = dev[(size_t)i];
        EgControl c;
        memcpy(&c, span_copy(res, Lay.ctl, D.ctl), sizeof c);
        eg_result_control(c, G[(size_t)i].runs, (int)G[(size_t)i].Y.l_blocks(), r[i]);
        memcpy(r[i].Scw, span_copy(res, Lay.ctl, D.est), bytes_of(D.est, (size_t)D.nv));
        memcpy(r[i].Tiw, span_copy(res, Lay.ctl, D.Tiw), bytes_of(D.Tiw, 16 * (size_t)D.nv));
        if (D.np > 0) memcpy(r[i].Xw, span_copy(res, Lay.ctl, D.Xw_out), bytes_of(D.Xw_out, 3 * (size_t)D.np));
    }
    return AOS2_OK;
}

float aos2_optimize_essential_graph_last_device_ms(const aos2_lba_t *s) { return s ? s->last_essential_graph_ms : 0.f; }

int aos2_debug_essential_graph_profile(aos2_lba_t *s, int on, float *family_ms)
{
    return LaunchProfiler::entry(s, &aos2_lba::eg_profile, &aos2_lba::eg_family_ms, on, family_ms);
}

int aos2_debug_essential_graph_host(const aos2_essential_graph_problem_t *p, aos2_essential_graph_result_t *r, int n_problems)
{
    if (int st = eg_check(p, r, n_problems, kEgHostMaxVertices)) return st;
    for (int i = 0; i < n_problems; ++i) {
        EgHostGraph G;
        eg_indices(p[i], G);
        if (G.runs && !eg_symbolic(G.nf, G.hi, G.lo, kEgArenaMax, G.Y)) {
            set_error("problem %d: the factor does not fit", i);
            return AOS2_ERR_EG_MEMORY;
        }
        eg_host_one(p[i], G, r[i]);
    }
    return AOS2_OK;
}

int aos2_debug_essential_graph_arith_host(int what, const double *in, int n, double *out)
{
    if (what < 0 || what > 2 || n < 0 || (n > 0 && (!in || !out))) {
        set_error("bad argument (what 0..2, n >= 0, the arrays)");
        return AOS2_ERR_ARG;
    }
    for (int i = 0; i < n; ++i) {
        if (what == 0)
            eg_log(eg_sim3(in)[i], out + 7 * (size_t)i);
        else if (what == 1) {
            const Sim3d *S = eg_sim3(in) + 3 * (size_t)i;
            Sim3d inv;
            so_inverse(S[2], inv);
            eg_residual(S[0], S[1], inv, out + 7 * (size_t)i);
        } else
            eg_lu3_solve(in + 12 * (size_t)i, in + 12 * (size_t)i + 9, out + 3 * (size_t)i);
    }
    return AOS2_OK;
}

int aos2_debug_essential_graph_solve_device(aos2_lba_t *s, int n_blocks, int n_off, const int32_t *rows, const int32_t *cols, const double *val,
                                            const double *diag, const double *b, double lambda, double *x, int32_t *ok, int32_t *l_blocks)
{
    return block_solve_tap<7, k_eg_factor_solve_tap>(s, kEgMaxVertices - 1, AOS2_ERR_EG_MEMORY, kEgArenaMax, n_blocks, n_off, rows, cols, val, diag, b,
                                                     lambda, x, ok, l_blocks);
}

int aos2_debug_essential_graph_linearised_device(aos2_lba_t *s, const aos2_essential_graph_problem_t *p, double *J, double *E, double *H, double *b,
                                                 double *chi2, int32_t *l_blocks)
{
    if (!J || !E || !H || !b || !chi2 || !l_blocks) {
        set_error("bad argument (the outputs)");
        return AOS2_ERR_ARG;
    }
    EgTap T;
    int st = eg_tap_linearise(s, p, T);
    if (st) return st;
    const EgHostGraph &G = T.G[0];
    const EgDev &D = T.Lay.dev[0];
    const size_t ne = (size_t)D.ne, n7 = 7 * (size_t)D.sys.nf;
    std::vector<double> Hv((size_t)D.sys.n_slots * 49);
    EgControl c;
    hipStream_t q = s->stream;
    AOS2_HIP_CHECK(hipMemcpyAsync(J, D.J, bytes_of(D.J, 98 * ne), hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(E, D.E, bytes_of(D.E, 7 * ne), hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(Hv.data(), D.sys.H, bytes_of(D.sys.H, Hv.size()), hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(b, D.sys.b, bytes_of(D.sys.b, n7), hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(&c, D.ctl, sizeof c, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    AOS2_HIP_CHECK(hipGetLastError());
    block_dense<7>(G.Y, Hv.data(), false, H);   // a diagonal slot as it is stored
    chi2[0] = c.lm.currentChi;
    chi2[1] = c.chi2_initial;
    *l_blocks = (int32_t)G.Y.l_blocks();
    return AOS2_OK;
}

int aos2_debug_essential_graph_trial_device(aos2_lba_t *s, const aos2_essential_graph_problem_t *p, const double *x, const double *seed_d,
                                            const int32_t *seed_i, double *est_try, double *est, double *control_d, int32_t *control_i, double *sums)
{
    if (!x || !seed_d || !seed_i || !est_try || !est || !control_d || !control_i || !sums) {
        set_error("bad argument (x, the seeds, the outputs)");
        return AOS2_ERR_ARG;
    }
    EgTap T;
    int st = eg_tap_linearise(s, p, T);
    if (st) return st;
    const EgDev &D = T.Lay.dev[0];
    const size_t nv = (size_t)D.nv, n7 = 7 * (size_t)D.sys.nf;
    hipStream_t q = s->stream;
    EgControl c;
    AOS2_HIP_CHECK(hipMemcpyAsync(&c, D.ctl, sizeof c, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    c.running = c.open = 1;
    c.lm.lambda = seed_d[0];
    c.lm.currentChi = seed_d[1];
    c.lm.ni = seed_d[2];
    c.solved = seed_i[0];
    c.iterations = seed_i[1];
    c.qmax = seed_i[2];
    AOS2_HIP_CHECK(hipMemcpyAsync(D.ctl, &c, sizeof c, hipMemcpyHostToDevice, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(D.sys.x, x, bytes_of(D.sys.x, n7), hipMemcpyHostToDevice, q));
    hipLaunchKernelGGL(k_eg_trial_tap, dim3(1), dim3(kEgThreads), 0, q, T.Lay.dprobs, T.sums);
    AOS2_HIP_CHECK(hipMemcpyAsync(est_try, D.est_try, bytes_of(D.est_try, nv), hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(est, D.est, bytes_of(D.est, nv), hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(sums, T.sums, bytes_of(T.sums, 2), hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(&c, D.ctl, sizeof c, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    AOS2_HIP_CHECK(hipGetLastError());
    const double cd[6] = {c.lm.lambda, c.lm.ni, c.lm.currentChi, c.lm.iniChi, c.rho, c.chi2_initial};
    const int32_t ci[10] = {c.lm.nBad, c.qmax, c.open, c.running, c.solved, c.max_iterations, c.iterations, c.trials, c.rejected, c.accepted_first};
    memcpy(control_d, cd, sizeof cd);
    memcpy(control_i, ci, sizeof ci);
    return AOS2_OK;
}

}  // extern "C"
