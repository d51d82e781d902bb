// Block-sparse LDL^T in device memory for a symmetric system of B x B blocks, eliminated in ascending order without pivoting: the
// symbolic phase on the host (the pattern of L by the elimination tree, the destinations of every column's trailing update) and
// the one-workgroup right-looking factorisation with the solve.  B = 7: the pose graph of essential_graph.hip; B = 6: the reduced
// camera system of global_ba.hip.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "lba_math.h"
#include "wave_ops.h"

namespace aos2 {

constexpr int kBlockLdltThreads = 256;

// (A + lambda I) x = b in B x B blocks.  Slot k < nf is the diagonal block of column k, slot nf + p the block rowidx[p] of the column c
// with colptr[c] <= p < colptr[c + 1] (rows ascending, below the diagonal).  A block is B * B doubles, row-major.
struct BlockSystem {
    int32_t nf, n_slots;
    const int32_t *colptr, *rowidx;   // [nf + 1], [n_slots - nf]
    const int32_t *upd_ptr, *upd_dst; // column k with rows r_0 < .. < r_{m-1}: upd_dst[upd_ptr[k] + j m - j (j - 1) / 2 + (i - j)] = the slot of block (r_i, r_j), i >= j
    const double *H, *b;              // [n_slots][B * B], [B nf]
    double *L, *y, *x;                // the factor (same slots), the right-hand side on its way, the solution
};

// LDL^T of a symmetric B x B (row-major, the lower triangle is read) in place: the unit lower factor below the diagonal, the pivots
// on it.  No pivoting.  false = a pivot is zero or NaN (LinearSolverEigen's failure); negative pivots pass, as they do there.
template <int B>
__host__ __device__ inline bool block_ldlt(double *a)
{
    for (int j = 0; j < B; ++j) {
        const double d = a[j * B + j];
        if (!(d == d) || d == 0) return false;
        const double rd = 1.0 / d;
        double w[B];
        for (int r = j + 1; r < B; ++r) {
            w[r] = a[r * B + j];
            a[r * B + j] = w[r] * rd;
        }
        for (int r = j + 1; r < B; ++r)
            for (int c = j + 1; c <= r; ++c) a[r * B + c] -= a[r * B + j] * w[c];
    }
    return true;
}

// The factorisation and the solve, one workgroup of kBlockLdltThreads per system, right-looking.  With A = L D L^T, L's diagonal
// blocks the unit lower factors Ld_k of the B x B LDL^T and D the pivots, column k is
//   1. Ld_k, D_k of the diagonal block (one thread, in LDS); z_k = Ld_k^-1 y_k
//   2. L_rk = A_rk Ld_k^-T D_k^-1, a thread per row of a block; y_r -= L_rk z_k
//   3. A_(ri, rj) -= L_(ri, k) D_k L_(rj, k)^T for every pair of rows of the column, a thread per entry
// and afterwards x_k = Ld_k^-T (D_k^-1 z_k - sum over the column's rows of L_rk^T x_r) for k descending.  A zero or NaN pivot ends
// it: solved = 0 and x keeps its values.
template <int B>
__device__ __forceinline__ void block_factor_solve(const BlockSystem &S, double lambda, int32_t *solved)
{
    constexpr int BB = B * B;
    static_assert(B <= 8, "the back substitution sums component a in row a of 16 lanes of two waves");
    __shared__ double D[BB], z[B], sums[8];
    __shared__ int fail;
    const int tid = threadIdx.x, nf = S.nf;
    const size_t nL = (size_t)S.n_slots * BB, nD = (size_t)nf * BB;
    for (size_t i = tid; i < nL; i += kBlockLdltThreads) {
        double v = S.H[i];
        if (i < nD && (i % BB) % (B + 1) == 0) v += lambda;
        S.L[i] = v;
    }
    for (int i = tid; i < B * nf; i += kBlockLdltThreads) S.y[i] = S.b[i];
    if (tid == 0) fail = 0;
    __syncthreads();
    for (int k = 0; k < nf; ++k) {
        if (tid < BB) D[tid] = S.L[(size_t)k * BB + tid];
        __syncthreads();
        if (tid == 0) {
            if (!block_ldlt<B>(D)) fail = 1;
            else {
                double zz[B];
                for (int r = 0; r < B; ++r) {
                    double s = S.y[B * k + r];
                    for (int m = 0; m < r; ++m) s -= D[r * B + m] * zz[m];
                    zz[r] = s;
                    z[r] = s;
                }
                for (int r = 0; r < B; ++r) S.y[B * k + r] = zz[r] / D[r * B + r];
            }
        }
        __syncthreads();
        if (fail) break;
        if (tid < BB) S.L[(size_t)k * BB + tid] = D[tid];
        const int p0 = S.colptr[k], m = S.colptr[k + 1] - p0;
        for (int it = tid; it < m * B; it += kBlockLdltThreads) {
            const int i = it / B, a = it % B;
            double *blk = S.L + (size_t)(nf + p0 + i) * BB + a * B;
            double w[B];
            for (int c = 0; c < B; ++c) {
                double s = blk[c];
                for (int q = 0; q < c; ++q) s -= w[q] * D[c * B + q];
                w[c] = s;
            }
            double dot = 0;
            for (int c = 0; c < B; ++c) {
                const double l = w[c] / D[c * B + c];
                blk[c] = l;
                dot += l * z[c];
            }
            S.y[B * S.rowidx[p0 + i] + a] -= dot;
        }
        __syncthreads();
        const int32_t *dst = S.upd_dst + S.upd_ptr[k];
        for (int j = 0; j < m; ++j) {
            const double *Lj = S.L + (size_t)(nf + p0 + j) * BB;
            const int base = j * m - j * (j - 1) / 2;
            for (int it = tid; it < (m - j) * BB; it += kBlockLdltThreads) {
                const int i = j + it / BB, ent = it % BB, a = ent / B, b = ent % B;
                const double *Li = S.L + (size_t)(nf + p0 + i) * BB + a * B;
                double s = 0;
                for (int c = 0; c < B; ++c) s += (Li[c] * D[c * B + c]) * Lj[b * B + c];
                S.L[(size_t)dst[base + (i - j)] * BB + ent] -= s;
            }
        }
        __syncthreads();
    }
    const bool ok = !fail;
    if (ok) {
        const int a = tid >> 4, l = tid & 15;
        for (int k = nf - 1; k >= 0; --k) {
            const int p0 = S.colptr[k], m = S.colptr[k + 1] - p0;
            if (tid < 128) {   // two whole waves: row a < B of 16 lanes sums component a, a fixed lane of the row keeps it
                double s = 0;
                if (a < B)
                    for (int t = l; t < m * B; t += 16) {
                        const int i = t / B, c = t % B;
                        s += S.L[(size_t)(nf + p0 + i) * BB + c * B + a] * S.x[B * S.rowidx[p0 + i] + c];
                    }
                s = row_sum_f64(s);
                if (l == 0) sums[a] = s;
            }
            __syncthreads();
            if (tid == 0) {
                const double *Ld = S.L + (size_t)k * BB;
                double xv[B];
                for (int r = B - 1; r >= 0; --r) {
                    double s = S.y[B * k + r] - sums[r];
                    for (int q = r + 1; q < B; ++q) s -= Ld[q * B + r] * xv[q];
                    xv[r] = s;
                }
                for (int r = 0; r < B; ++r) S.x[B * k + r] = xv[r];
            }
            __syncthreads();
        }
    }
    if (tid == 0) *solved = ok;
}

// ---------------------------------------------------------------------------------------------- the symbolic phase (host)
struct BlockSymbolic {
    int nf = 0;
    std::vector<int32_t> colptr, rowidx, upd_ptr, upd_dst;
    size_t l_blocks() const { return rowidx.size(); }
    int slot(int row, int col) const   // row > col, present in the pattern of L
    {
        const int32_t *b = rowidx.data() + colptr[col], *e = rowidx.data() + colptr[col + 1];
        return nf + (int)(std::lower_bound(b, e, row) - rowidx.data());
    }
};

// the pattern of L for the lower-triangle blocks (hi[i], lo[i]) eliminated in ascending order: a column's rows are those of A's
// column and, but for the column itself, those of every child in the elimination tree (parent = the first row of the column).
// false: the factor (blocks of block_doubles doubles, kept twice: A and L) and its update table would take more than max_bytes.
inline bool block_symbolic(int nf, const std::vector<int32_t> &hi, const std::vector<int32_t> &lo, size_t block_doubles, size_t max_bytes,
                           BlockSymbolic &Y)
{
    Y.nf = nf;
    std::vector<std::vector<int32_t>> rows((size_t)nf);
    for (size_t i = 0; i < hi.size(); ++i) rows[(size_t)lo[i]].push_back(hi[i]);
    size_t n_l = 0, n_upd = 0;
    for (int k = 0; k < nf; ++k) {
        std::vector<int32_t> &r = rows[(size_t)k];
        std::sort(r.begin(), r.end());
        r.erase(std::unique(r.begin(), r.end()), r.end());
        if (r.size() > 1) {
            std::vector<int32_t> &par = rows[(size_t)r[0]];
            par.insert(par.end(), r.begin() + 1, r.end());
        }
        n_l += r.size();
        n_upd += r.size() * (r.size() + 1) / 2;
        if ((n_l + (size_t)nf) * block_doubles * 8 * 2 + n_upd * 4 > max_bytes) return false;
    }
    Y.colptr.assign((size_t)nf + 1, 0);
    Y.rowidx.clear();
    Y.rowidx.reserve(n_l);
    for (int k = 0; k < nf; ++k) {
        Y.rowidx.insert(Y.rowidx.end(), rows[(size_t)k].begin(), rows[(size_t)k].end());
        Y.colptr[(size_t)k + 1] = (int32_t)Y.rowidx.size();
    }
    Y.upd_ptr.assign((size_t)nf + 1, 0);
    Y.upd_dst.clear();
    Y.upd_dst.reserve(n_upd);
    for (int k = 0; k < nf; ++k) {
        const std::vector<int32_t> &r = rows[(size_t)k];
        for (size_t j = 0; j < r.size(); ++j) {
            Y.upd_dst.push_back(r[j]);
            for (size_t i = j + 1; i < r.size(); ++i) Y.upd_dst.push_back(Y.slot(r[i], r[j]));
        }
        Y.upd_ptr[(size_t)k + 1] = (int32_t)Y.upd_dst.size();
    }
    return true;
}

// The slots of a system as a dense (B nf) x (B nf) row-major matrix, both triangles.  A slot below the diagonal goes to its place
// and, transposed, to the mirrored one.  A diagonal slot is copied as it is stored; with diag_lower it is given by its lower
// triangle, which is mirrored.
template <int B>
inline void block_dense(const BlockSymbolic &Y, const double *slots, bool diag_lower, double *out)
{
    const size_t nf = (size_t)Y.nf, n = B * nf;
    std::fill(out, out + n * n, 0.0);
    for (size_t sl = 0; sl < nf + Y.l_blocks(); ++sl) {
        const bool diag = sl < nf;
        size_t row = sl, col = sl;
        if (!diag) {
            const int p = (int)(sl - nf);
            row = (size_t)Y.rowidx[(size_t)p];
            col = (size_t)(std::upper_bound(Y.colptr.begin(), Y.colptr.end(), p) - Y.colptr.begin()) - 1;
        }
        for (size_t a = 0; a < B; ++a)
            for (size_t c = 0; c < (diag && diag_lower ? a + 1 : B); ++c) {
                const double v = slots[sl * B * B + a * B + c];
                out[(B * row + a) * n + B * col + c] = v;
                if (!diag || diag_lower) out[(B * col + c) * n + B * row + a] = v;
            }
    }
}

// ---------------------------------------------------------------------------------------------- the solve tap (host)
// block_factor_solve<B> alone on a system given by its diagonal blocks and the triplets of blocks below the diagonal (repeated
// triplets add up), through the real symbolic phase: aos2_debug_essential_graph_solve_device, aos2_debug_global_ba_solve_device.
// kKernel is the entry's one-workgroup kernel around block_factor_solve<B>.
template <int B, void (*kKernel)(BlockSystem, double, int32_t *)>
int block_solve_tap(aos2_lba *s, int max_blocks, int err_memory, size_t max_bytes, int n_blocks, int n_off, const int32_t *rows, const int32_t *cols,
                    const double *val, const double *diag, const double *b, double lambda, double *x, int32_t *ok, int32_t *l_blocks)
{
    constexpr size_t BB = B * B;
    bool good = s && n_blocks >= 1 && n_blocks <= max_blocks && n_off >= 0 && diag && b && x && ok && l_blocks && (n_off == 0 || (rows && cols && val));
    for (int i = 0; good && i < n_off; ++i) good = cols[i] >= 0 && rows[i] > cols[i] && rows[i] < n_blocks;
    if (!good) {
        set_error("bad argument (1..%d blocks, triplets of the lower triangle, the arrays)", max_blocks);
        return AOS2_ERR_ARG;
    }
    BlockSymbolic Y;
    if (!block_symbolic(n_blocks, std::vector<int32_t>(rows, rows + n_off), std::vector<int32_t>(cols, cols + n_off), BB, max_bytes, Y)) {
        set_error("the factor does not fit");
        return err_memory;
    }
    const size_t n_slots = (size_t)n_blocks + Y.l_blocks(), nx = B * (size_t)n_blocks;
    std::vector<double> Hv(n_slots * BB, 0.0);
    memcpy(Hv.data(), diag, sizeof(double) * BB * (size_t)n_blocks);
    for (int i = 0; i < n_off; ++i) {
        double *dst = Hv.data() + (size_t)Y.slot(rows[i], cols[i]) * BB;
        for (size_t k = 0; k < BB; ++k) dst[k] += val[(size_t)i * BB + k];
    }
    int st = lba_handle_init(s);
    if (st) return st;
    HostArena H;
    BlockSystem S;
    int32_t *d_ok = nullptr;
    S.nf = n_blocks;
    S.n_slots = (int32_t)n_slots;
    H.in(S.colptr, Y.colptr);
    H.in(S.rowidx, Y.rowidx);
    H.in(S.upd_ptr, Y.upd_ptr);
    H.in(S.upd_dst, Y.upd_dst);
    H.in(S.H, Hv);
    H.in(S.b, b, nx);
    H.in(S.x, (const double *)x, nx);
    const size_t in_bytes = H.host_size;
    H.room(d_ok, 1);
    H.room(S.L, Hv.size());
    H.room(S.y, nx);
    if ((st = s->arena.alloc(H.size + 256))) return st;
    H.bind(s->arena.p);
    hipStream_t q = s->stream;
    AOS2_HIP_CHECK(hipMemcpyAsync(s->arena.p, H.data(), in_bytes, hipMemcpyHostToDevice, q));
    hipLaunchKernelGGL(kKernel, dim3(1), dim3(kBlockLdltThreads), 0, q, S, lambda, d_ok);
    AOS2_HIP_CHECK(hipMemcpyAsync(x, S.x, sizeof(double) * nx, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(ok, d_ok, sizeof(int32_t), hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    AOS2_HIP_CHECK(hipGetLastError());
    *l_blocks = (int32_t)Y.l_blocks();
    return AOS2_OK;
}

// ---------------------------------------------------------------------------------------------- the host taps' solver
// the scalar system in skyline storage: row i keeps columns first[i] .. i
struct SkylineLdlt {
    int n = 0;
    std::vector<int> first;
    std::vector<size_t> off;
    std::vector<double> A, L, d, tmp;
    double &a(std::vector<double> &M, int i, int j) { return M[off[(size_t)i] + (size_t)(j - first[(size_t)i])]; }

    // nf blocks of B x B, the blocks (hi[i], lo[i]) below the diagonal
    void shape(int nf, const std::vector<int32_t> &hi, const std::vector<int32_t> &lo, int B)
    {
        std::vector<int> minblk((size_t)nf);
        for (int h = 0; h < nf; ++h) minblk[(size_t)h] = h;
        for (size_t i = 0; i < hi.size(); ++i) minblk[(size_t)hi[i]] = std::min(minblk[(size_t)hi[i]], (int)lo[i]);
        n = B * nf;
        first.resize((size_t)n);
        off.resize((size_t)n + 1);
        size_t total = 0;
        for (int i = 0; i < n; ++i) {
            first[(size_t)i] = B * minblk[(size_t)(i / B)];
            off[(size_t)i] = total;
            total += (size_t)(i - first[(size_t)i] + 1);
        }
        off[(size_t)n] = total;
        A.assign(total, 0.0);
        L.assign(total, 0.0);
        d.assign((size_t)n, 0.0);
        tmp.assign((size_t)n, 0.0);
    }
    // (A + lambda I) x = b by LDL^T inside the envelope, row by row; false = a zero or NaN pivot, x keeps its values
    bool solve(double lambda, const std::vector<double> &b, std::vector<double> &x)
    {
        L = A;
        for (int i = 0; i < n; ++i) {
            const int fi = first[(size_t)i];
            for (int j = fi; j < i; ++j) {
                double s = a(L, i, j);
                for (int k = std::max(fi, first[(size_t)j]); k < j; ++k) s -= tmp[(size_t)k] * a(L, j, k);
                tmp[(size_t)j] = s;
            }
            double di = a(L, i, i) + lambda;
            for (int j = fi; j < i; ++j) {
                const double l = tmp[(size_t)j] / d[(size_t)j];
                a(L, i, j) = l;
                di -= tmp[(size_t)j] * l;
            }
            if (!(di == di) || di == 0) return false;
            d[(size_t)i] = di;
        }
        std::vector<double> y((size_t)n);
        for (int i = 0; i < n; ++i) {
            double s = b[(size_t)i];
            for (int j = first[(size_t)i]; j < i; ++j) s -= a(L, i, j) * y[(size_t)j];
            y[(size_t)i] = s;
        }
        for (int i = 0; i < n; ++i) y[(size_t)i] /= d[(size_t)i];
        for (int i = n - 1; i >= 0; --i) {
            const double xi = y[(size_t)i];
            for (int j = first[(size_t)i]; j < i; ++j) y[(size_t)j] -= a(L, i, j) * xi;
        }
        x = y;
        return true;
    }
};

}  // namespace aos2
