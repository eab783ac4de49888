// K_clean: frame censoring and confound regression in front of K_corr (fcd_corr.hip).
//
// Per subject, over its KEPT frames only (frame_mask; a dropped frame is never loaded into a sum: every kernel selects
// on the mask, none multiplies by it):
//   1. every region row y and every confound row x is centred by its mean over the kept frames (the implied intercept);
//   2. a confound constant over the kept frames is dropped; the others are scaled to unit norm;
//   3. collinear confounds are dropped by diagonally pivoted Cholesky of their Gram matrix (remaining squared norm below
//      1e-10 of the unit norm: not used); rank = columns used, dof = n_kept - 1 - rank;
//   4. resid = y_c - beta^T x_c, beta from the normal equations of the used columns, written to positions 0 .. n_kept - 1
//      of the row in frame order, exact zeros behind them;
//   5. a row that is constant, holds a non-finite kept sample, or whose residual sum of squares (from the residual
//      itself) is <= 1e-20 of its centred sum of squares is written as zeros; so is every row of a subject with dof < 2
//      or with a non-finite kept sample in a confound (such a subject reports rank 0: nothing was solved).
// K_corr on the zero-padded residuals then gives their Pearson correlation: the rows have mean 0 over n_kept frames, the
// zeros add nothing to any sum and the 1 / (T - 1) of the covariance cancels.  A zero row comes out as NaN edges there.
//
// Kernels (all on the caller's stream, fixed reduction orders, no floating-point atomics: two calls agree bit for bit):
//   clean_index_kernel    one workgroup per subject: prefix sum of the mask -> list of kept frames, n_kept
//   clean_moments_kernel  one wave per (subject, row) of the Q + Nreg rows: mean, centred sum of squares from a second
//                         read, min == max, non-finite samples, unit scale of a confound
//   clean_gram_kernel     Q x (Q + Nreg) normal equations per subject: v_mfma_f64_16x16x4_f64 tiles over LDS-staged,
//                         double-buffered 64 x 16 panels as corr_gram_kernel stages them; the gather through the frame
//                         list, centring and scaling happen on the way into LDS.  One workgroup per (subject, 64 columns)
//   clean_chol_kernel     one workgroup per subject: pivoted Cholesky of the Q x Q matrix in LDS with the drop rule, info
//   clean_beta_kernel     one workgroup per (subject, 64 regions): beta by forward / back substitution, four lanes per column
//   clean_resid_kernel    one wave per (subject, 64 kept frames, 64 regions): the lane keeps its frame's Q centred confound
//                         values in registers, beta rows arrive wave-uniform; coalesced 512-byte stores, tail zero-filled
//   clean_finish_kernel   one wave per (subject, region): residual sum of squares of the written row, rule 5
#include "fcd_common.h"

#include <float.h>

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int QMAX = 64;                 // confounds per subject (the Cholesky's LDS image, the resid kernel's registers)
constexpr int ROW_CONST = 1, ROW_NONFINITE = 2;
constexpr double DROP_TOL = 1e-10;       // remaining squared norm of a unit-norm confound below which it is not used
constexpr double RSS_TOL = 1e-20;        // residual sum of squares / centred sum of squares at or below which a row has no residual

// Rows of a subject are numbered confounds first: r < Q confound r, else region r - Q.
__device__ __forceinline__ const double *clean_row(const double *ts, const double *cf, int64_t s, int r, int Nreg, int Q, int T) {
    return r < Q ? cf + ((int64_t)s * Q + r) * T : ts + ((int64_t)s * Nreg + (r - Q)) * T;
}

__global__ __launch_bounds__(256) void clean_index_kernel(const uint8_t *__restrict__ mask, int T, int *__restrict__ idx,
                                                          int *__restrict__ nk) {
    __shared__ int wsum[4];
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int base = 0;
    for (int64_t t0 = 0; t0 < T; t0 += 256) {
        const int64_t t = t0 + tid;
        const bool keep = t < T && (mask ? mask[s * T + t] != 0 : true);
        const unsigned long long b = __ballot(keep);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(b);
        __syncthreads();
        int off = base;
        for (int v = 0; v < w; ++v) off += wsum[v];
        if (keep) idx[s * T + off + before] = (int)t;
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) nk[s] = base;
}

__global__ __launch_bounds__(256) void clean_moments_kernel(const double *__restrict__ ts, const double *__restrict__ cf,
                                                            const int *__restrict__ idx, const int *__restrict__ nk, int64_t rows,
                                                            int Nreg, int Q, int T, double *__restrict__ mean,
                                                            double *__restrict__ ss, double *__restrict__ scale,
                                                            int *__restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int R = Nreg + Q;
    const int64_t s = row / R;
    const int r = (int)(row % R);
    const double *x = clean_row(ts, cf, s, r, Nreg, Q, T);
    const int *ix = idx + s * T;
    const int n = nk[s];
    double sum = 0.0;
#pragma unroll 4
    for (int j = lane; j < n; j += 64) sum += x[ix[j]];
    sum = fcd_wave_sum(sum);
    const double mu = sum / (double)n;
    double q = 0.0, mn = DBL_MAX, mx = -DBL_MAX;
    int bad = 0;
#pragma unroll 4
    for (int j = lane; j < n; j += 64) {
        const double v = x[ix[j]];
        const double d = v - mu;
        q += d * d;
        mn = fmin(mn, v);
        mx = fmax(mx, v);
        bad |= !(fabs(v) <= DBL_MAX);
    }
    q = fcd_wave_sum(q);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o, 64));
        mx = fmax(mx, __shfl_xor(mx, o, 64));
    }
    bad = __any(bad);
    int f = 0;
    if (bad) f = ROW_NONFINITE;
    else if (n == 0 || mn == mx) f = ROW_CONST;
    if (lane == 0) {
        mean[row] = f ? 0.0 : mu;
        ss[row] = f ? 0.0 : q;
        double sc = 0.0;                                   // (a dropped confound: its row of the Gram matrix is zero)
        if (!f) sc = r < Q ? 1.0 / sqrt(q) : 1.0;
        if (!(sc <= DBL_MAX)) sc = 0.0;
        scale[row] = sc;
        flag[row] = f;
    }
}

// Normal equations.  grid = (blocks of 64 columns of [confounds | regions], subjects); block = 4 waves, wave (wr, wc) owns
// the 2 x 2 MFMA tiles (2 wr + {0,1}, 2 wc + {0,1}) of the 64 x 64 block: rows = confounds, columns = this block's rows of
// the subject.  K = the kept frames in steps of 16, panels padded to 18 doubles and double-buffered exactly as in
// corr_gram_kernel (fcd_corr.hip), whose fragment layout this follows.  A flagged row is staged as zeros.
constexpr int GB = 64, GK = 16, GLD = 18;
__global__ __launch_bounds__(256) void clean_gram_kernel(const double *__restrict__ ts, const double *__restrict__ cf,
                                                         const int *__restrict__ idx, const int *__restrict__ nk,
                                                         const double *__restrict__ mean, const double *__restrict__ scale,
                                                         int Nreg, int Q, int T, double *__restrict__ G) {
    __shared__ __attribute__((aligned(16))) double pa[2][GB * GLD], pb[2][GB * GLD];
    const int64_t s = blockIdx.y;
    const int J = blockIdx.x, R = Nreg + Q;
    const int n = nk[s];
    const int *ix = idx + s * T;
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const int wr = w >> 1, wc = w & 1;
    const int prow = tid >> 3, pp = tid & 7;
    const double *xa[2], *xb[2];
    double ma[2], mb[2], sa[2], sb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ga = prow + 32 * h, gb = J * GB + prow + 32 * h;
        const bool va = ga < Q, vb = gb < R;
        xa[h] = clean_row(ts, cf, s, va ? ga : Q, Nreg, Q, T);         // (row Q = region 0 always exists)
        xb[h] = clean_row(ts, cf, s, vb ? gb : Q, Nreg, Q, T);
        ma[h] = va ? mean[s * R + ga] : 0.0;
        mb[h] = vb ? mean[s * R + gb] : 0.0;
        sa[h] = va ? scale[s * R + ga] : 0.0;                          // 0: constant, non-finite or absent row
        sb[h] = vb ? scale[s * R + gb] : 0.0;
    }
    double2 ra[2], rb[2];
    auto fetch = [&](int k0) {
        const int k = k0 + 2 * pp;
        const bool in0 = k < n, in1 = k + 1 < n;
        const int t0 = in0 ? ix[k] : 0, t1 = in1 ? ix[k + 1] : 0;      // (frame 0 is loaded and thrown away)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double a0 = xa[h][t0], a1 = xa[h][t1], b0 = xb[h][t0], b1 = xb[h][t1];
            ra[h].x = (in0 && sa[h] != 0.0) ? (a0 - ma[h]) * sa[h] : 0.0;
            ra[h].y = (in1 && sa[h] != 0.0) ? (a1 - ma[h]) * sa[h] : 0.0;
            rb[h].x = (in0 && sb[h] != 0.0) ? (b0 - mb[h]) * sb[h] : 0.0;
            rb[h].y = (in1 && sb[h] != 0.0) ? (b1 - mb[h]) * sb[h] : 0.0;
        }
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<double2 *>(&pa[buf][(prow + 32 * h) * GLD + 2 * pp]) = ra[h];
            *reinterpret_cast<double2 *>(&pb[buf][(prow + 32 * h) * GLD + 2 * pp]) = rb[h];
        }
    };
    double4_t acc[2][2];
    bool on[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};
            on[a][b] = ((2 * wr + a) * 16 < Q) && (J * GB + (2 * wc + b) * 16 < R);
        }
    const bool any_on = on[0][0] || on[0][1] || on[1][0] || on[1][1];
    const int i16 = l & 15, kq = l >> 4;
    const int steps = (n + GK - 1) / GK;
    if (steps > 0) {
        fetch(0);
        put(0);
    }
    __syncthreads();
    for (int st = 0; st < steps; ++st) {
        const int cur = st & 1;
        if (st + 1 < steps) fetch((st + 1) * GK);
        if (any_on) {
            const double *A = pa[cur];
            const double *B = pb[cur];
#pragma unroll
            for (int g = 0; g < GK / 4; ++g) {
                double fa[2], fb[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) fa[a] = A[((2 * wr + a) * 16 + i16) * GLD + g * 4 + kq];
#pragma unroll
                for (int b = 0; b < 2; ++b) fb[b] = B[((2 * wc + b) * 16 + i16) * GLD + g * 4 + kq];
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        if (on[a][b]) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
            }
        }
        if (st + 1 < steps) put(cur ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (!on[a][b]) continue;
            const int col = J * GB + (2 * wc + b) * 16 + i16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = (2 * wr + a) * 16 + kq + 4 * r;
                if (q < Q && col < R) G[((int64_t)s * QMAX + q) * R + col] = acc[a][b][r];
            }
        }
}

// One workgroup per subject.  A (LDS, rows padded to 65) holds the Gram matrix of the unit-scaled confounds and becomes
// its pivoted Cholesky factor in place: step k takes the column p with the largest remaining diagonal (ties: the lowest
// index), stops when that is below DROP_TOL, and leaves L[j][k] in A[j][p] for every column j not taken yet -- so
// L[piv[k]][m] = A[piv[k]][piv[m]] for m <= k, written out as the packed triangle Lc (S, LCN) with piv (S, 64).
constexpr int LCN = QMAX * (QMAX + 1) / 2, ALD = QMAX + 1;
__global__ __launch_bounds__(256) void clean_chol_kernel(const double *__restrict__ G, const int *__restrict__ flag,
                                                         const int *__restrict__ nk, int Nreg, int Q, double *__restrict__ Lc,
                                                         int *__restrict__ piv_out, int *__restrict__ info, int *__restrict__ sflag) {
    __shared__ double A[QMAX * ALD];
    __shared__ int piv[QMAX], taken[QMAX];
    __shared__ int sh_p;
    __shared__ double sh_d;
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, R = Nreg + Q;
    const int n = nk[s];
    int bad = 0;
    if (tid < Q) bad = (flag[s * R + tid] & ROW_NONFINITE) != 0;
    bad = __syncthreads_or(bad);
    int rank = 0;
    if (Q > 0 && !bad) {
        for (int e = tid; e < Q * Q; e += 256) {
            const int i = e / Q, j = e % Q;        // (the lower triangle, mirrored)
            A[i * ALD + j] = G[((int64_t)s * QMAX + (i > j ? i : j)) * R + (i > j ? j : i)];
        }
        if (tid < QMAX) taken[tid] = 0;
        __syncthreads();
        for (int k = 0; k < Q; ++k) {
            if (tid < 64) {
                double d = (tid < Q && !taken[tid]) ? A[tid * ALD + tid] : -1.0;
                if (!(d == d)) d = -1.0;
                int i = tid;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double od = __shfl_xor(d, o, 64);
                    const int oi = __shfl_xor(i, o, 64);
                    if (od > d || (od == d && oi < i)) {
                        d = od;
                        i = oi;
                    }
                }
                if (tid == 0) {
                    sh_p = i;
                    sh_d = d;
                }
            }
            __syncthreads();
            const int p = sh_p;
            const double dp = sh_d;
            if (!(dp >= DROP_TOL)) break;                 // (uniform)
            const double lpp = sqrt(dp);
            if (tid < Q && !taken[tid] && tid != p) A[tid * ALD + p] = A[tid * ALD + p] / lpp;
            __syncthreads();
            for (int e = tid; e < Q * Q; e += 256) {
                const int i = e / Q, j = e % Q;
                if (i != p && j != p && !taken[i] && !taken[j]) A[i * ALD + j] -= A[i * ALD + p] * A[j * ALD + p];
            }
            __syncthreads();
            if (tid == 0) {
                A[p * ALD + p] = lpp;
                taken[p] = 1;
                piv[k] = p;
            }
            ++rank;
            __syncthreads();
        }
        for (int e = tid; e < rank * rank; e += 256) {
            const int k = e / rank, m = e % rank;
            if (m <= k) Lc[s * LCN + k * (k + 1) / 2 + m] = A[piv[k] * ALD + piv[m]];
        }
        if (tid < rank) piv_out[s * QMAX + tid] = piv[tid];
    }
    if (tid == 0) {
        const int dof = n - 1 - rank;
        info[s * 3 + 0] = n;
        info[s * 3 + 1] = rank;
        info[s * 3 + 2] = dof;
        sflag[s] = bad || dof < 2;
    }
}

// beta by forward and back substitution.  grid = (blocks of 64 region columns, subjects).  Four consecutive lanes share a
// column: lane part takes the terms m = part (mod 4) of every sum, the four partial sums meet in a fixed tree, lane 0 of the
// four divides and writes y_k into the LDS tile Y[k][column] for the steps behind it.  beta (S, Nreg, 64): entry q of a
// region's row = its coefficient on the centred, UNscaled confound q; 0 for a confound not used.  A zeroed subject's
// beta is never read and is not written.
__global__ __launch_bounds__(256) void clean_beta_kernel(const double *__restrict__ G, const double *__restrict__ Lc,
                                                         const int *__restrict__ piv_in, const int *__restrict__ info,
                                                         const int *__restrict__ sflag, const double *__restrict__ scale, int Nreg,
                                                         int Q, double *__restrict__ beta) {
    __shared__ double L[LCN];
    __shared__ double Y[QMAX * ALD];
    __shared__ int pv[QMAX], inv[QMAX];
    const int64_t s = blockIdx.y;
    if (sflag[s]) return;
    const int tid = threadIdx.x, R = Nreg + Q, rank = info[s * 3 + 1];
    const int c0 = blockIdx.x * 64, cl = tid >> 2, part = tid & 3;
    for (int e = tid; e < rank * (rank + 1) / 2; e += 256) L[e] = Lc[s * LCN + e];
    if (tid < QMAX) inv[tid] = -1;
    __syncthreads();
    if (tid < rank) {
        const int p = piv_in[s * QMAX + tid];
        pv[tid] = p;
        inv[p] = tid;
    }
    __syncthreads();
    for (int e = tid; e < rank * 64; e += 256) {
        const int k = e >> 6, c = c0 + (e & 63);
        Y[k * ALD + (e & 63)] = c < Nreg ? G[((int64_t)s * QMAX + pv[k]) * R + Q + c] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < rank; ++k) {
        double p = 0.0;
        for (int m = part; m < k; m += 4) p += L[k * (k + 1) / 2 + m] * Y[m * ALD + cl];
        p += __shfl_xor(p, 1, 64);
        p += __shfl_xor(p, 2, 64);
        if (part == 0) Y[k * ALD + cl] = (Y[k * ALD + cl] - p) / L[k * (k + 1) / 2 + k];
        __syncthreads();
    }
    for (int k = rank - 1; k >= 0; --k) {
        double p = 0.0;
        for (int m = k + 1 + part; m < rank; m += 4) p += L[m * (m + 1) / 2 + k] * Y[m * ALD + cl];
        p += __shfl_xor(p, 1, 64);
        p += __shfl_xor(p, 2, 64);
        if (part == 0) Y[k * ALD + cl] = (Y[k * ALD + cl] - p) / L[k * (k + 1) / 2 + k];
        __syncthreads();
    }
    for (int e = tid; e < 64 * QMAX; e += 256) {
        const int q = e & 63, c = c0 + (e >> 6);
        if (c < Nreg) {
            const int k = inv[q];
            beta[((int64_t)s * Nreg + c) * QMAX + q] = k >= 0 ? Y[k * ALD + (e >> 6)] * scale[s * R + q] : 0.0;
        }
    }
}

// Residuals, compacted.  grid = (tiles of 4 x 64 output positions, blocks of RC regions, subjects); wave w of a workgroup
// owns output positions j = 64 (4 blockIdx.x + w) + lane of RC rows.  The lane keeps the centred confound values of ITS
// kept frame in registers (QP of them; 0 beyond Q), the coefficients of a row are the same for the whole wave.
constexpr int RC = 64;
template <int QP>
__global__ __launch_bounds__(256) void clean_resid_kernel(const double *__restrict__ ts, const double *__restrict__ cf,
                                                          const int *__restrict__ idx, const int *__restrict__ nk,
                                                          const double *__restrict__ mean, const int *__restrict__ flag,
                                                          const int *__restrict__ sflag, const double *__restrict__ beta, int Nreg,
                                                          int Q, int T, double *__restrict__ resid) {
    constexpr int QA = QP > 0 ? QP : 1;
    __shared__ double bt[RC * QA];                               // the coefficients of this workgroup's rows: [row][q]
    const int64_t s = blockIdx.z;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c0 = blockIdx.y * RC, c1 = c0 + RC < Nreg ? c0 + RC : Nreg;
    if (QP > 0 && !sflag[s]) {                                   // (a zeroed subject has no beta)
        for (int e = threadIdx.x; e < (c1 - c0) * QA; e += 256)
            bt[e] = beta[((int64_t)s * Nreg + c0 + e / QA) * QMAX + e % QA];
    }
    __syncthreads();
    const int64_t j0 = ((int64_t)blockIdx.x * 4 + w) * 64;
    if (j0 >= T) return;
    const int64_t j = j0 + lane;
    const int R = Nreg + Q;
    const int n = nk[s];
    const bool live = !sflag[s] && j < n;                       // this lane writes a residual (else 0.0)
    const int t = live ? idx[s * T + j] : 0;
    double x[QA];
#pragma unroll
    for (int q = 0; q < QA; ++q) x[q] = 0.0;
    if (QP > 0) {
#pragma unroll
        for (int q = 0; q < QA; ++q)
            if (q < Q && live) x[q] = cf[((int64_t)s * Q + q) * T + t] - mean[s * R + q];
    }
#pragma unroll 2
    for (int c = c0; c < c1; ++c) {
        const int64_t row = (int64_t)s * Nreg + c;
        double out = 0.0;
        if (live && !flag[s * R + Q + c]) {
            const double yc = ts[row * T + t] - mean[s * R + Q + c];
            double a = 0.0;
            if (QP > 0) {
                const double *bq = bt + (c - c0) * QA;
#pragma unroll
                for (int q = 0; q < QA; ++q) a += bq[q] * x[q];
            }
            out = yc - a;
        }
        if (j < T) resid[row * T + j] = out;
    }
}

__global__ __launch_bounds__(256) void clean_finish_kernel(const int *__restrict__ nk, const double *__restrict__ ss,
                                                           const int *__restrict__ flag, const int *__restrict__ sflag, int64_t rows,
                                                           int Nreg, int Q, int T, double *__restrict__ resid) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t s = row / Nreg;
    const int c = (int)(row % Nreg), R = Nreg + Q;
    if (sflag[s] || flag[s * R + Q + c]) return;                // (written as zeros already)
    const int n = nk[s];
    double *x = resid + row * T;
    double q = 0.0;
    for (int j = lane; j < n; j += 64) q += x[j] * x[j];
    q = fcd_wave_sum(q);
    if (!(q > RSS_TOL * ss[s * R + Q + c]))
        for (int j = lane; j < n; j += 64) x[j] = 0.0;
}

}  // namespace

extern "C" int fcd_corr_clean(fcd_ctx *ctx, const double *ts, const double *confounds, const uint8_t *frame_mask, int64_t S,
                              int64_t Nreg, int64_t Q, int64_t T, double *resid, int32_t *info, fcd_stream stream) {
    if (!ctx || !ts || !resid || !info) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_corr_clean: null pointer");
    if (S < 1 || Nreg < 2 || T < 2) return fcd_fail(ctx, FCD_ERR_SHAPE, "need S >= 1, Nreg >= 2, T >= 2 (Nreg=%lld, T=%lld)", Nreg, T);
    if (Q < 0) return fcd_fail(ctx, FCD_ERR_SHAPE, "fcd_corr_clean: Q=%lld is negative", Q);
    if (Q > QMAX) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_corr_clean: Q=%lld confounds, at most 64", Q);
    if (S > 65535 || Nreg > 46340 || T > INT32_MAX) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_corr_clean: shape too large");
    if (Q > 0 && !confounds) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_corr_clean: Q=%lld but confounds is null", Q);
    const int64_t R = Nreg + Q, rows = S * R;
    if ((T + 255) / 256 > INT32_MAX || (rows + 3) / 4 > INT32_MAX) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_corr_clean: grid too large");
    hipStream_t st = (hipStream_t)stream;
    // workspace: G | beta | Lc | mean | ss | scale (doubles), then idx | n_kept | row flags | subject flags | piv (ints).
    // Nothing here outlives the call: fcd_corr_edges may regrow the workspace right afterwards.
    const size_t nG = Q ? (size_t)S * QMAX * R : 0, nB = Q ? (size_t)S * Nreg * QMAX : 0, nL = Q ? (size_t)S * LCN : 0;
    const size_t n_dbl = nG + nB + nL + 3 * (size_t)rows;
    const size_t n_int = (size_t)S * T + (size_t)S + (size_t)rows + (size_t)S + (size_t)S * QMAX;
    int rc = fcd_ws_reserve(ctx, n_dbl * sizeof(double) + n_int * sizeof(int));
    if (rc) return rc;
    double *G = (double *)ctx->ws.p, *beta = G + nG, *Lc = beta + nB, *mean = Lc + nL, *ss = mean + rows, *scale = ss + rows;
    int *idx = (int *)(scale + rows), *nk = idx + (size_t)S * T, *flag = nk + S, *sflag = flag + rows, *piv = sflag + S;
    const int N = (int)Nreg, Qi = (int)Q, Ti = (int)T;
    hipLaunchKernelGGL(clean_index_kernel, dim3((unsigned)S), dim3(256), 0, st, frame_mask, Ti, idx, nk);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(clean_moments_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, ts, confounds, idx, nk, rows, N, Qi, Ti,
                       mean, ss, scale, flag);
    FCD_LAUNCH_CHECK();
    if (Q > 0) {
        hipLaunchKernelGGL(clean_gram_kernel, dim3((unsigned)((R + GB - 1) / GB), (unsigned)S), dim3(256), 0, st, ts, confounds, idx, nk,
                           mean, scale, N, Qi, Ti, G);
        FCD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(clean_chol_kernel, dim3((unsigned)S), dim3(256), 0, st, G, flag, nk, N, Qi, Lc, piv, info, sflag);
    FCD_LAUNCH_CHECK();
    if (Q > 0) {
        hipLaunchKernelGGL(clean_beta_kernel, dim3((unsigned)((Nreg + 63) / 64), (unsigned)S), dim3(256), 0, st, G, Lc, piv, info, sflag,
                           scale, N, Qi, beta);
        FCD_LAUNCH_CHECK();
    }
    const dim3 rgrid((unsigned)((T + 255) / 256), (unsigned)((Nreg + RC - 1) / RC), (unsigned)S);
#define FCD_CLEAN_RESID(QP) \
    hipLaunchKernelGGL(clean_resid_kernel<QP>, rgrid, dim3(256), 0, st, ts, confounds, idx, nk, mean, flag, sflag, beta, N, Qi, Ti, resid)
    switch ((Q + 7) / 8) {                // QP: Q rounded up to a multiple of 8
    case 0: FCD_CLEAN_RESID(0); break;
    case 1: FCD_CLEAN_RESID(8); break;
    case 2: FCD_CLEAN_RESID(16); break;
    case 3: FCD_CLEAN_RESID(24); break;
    case 4: FCD_CLEAN_RESID(32); break;
    case 5: FCD_CLEAN_RESID(40); break;
    case 6: FCD_CLEAN_RESID(48); break;
    case 7: FCD_CLEAN_RESID(56); break;
    default: FCD_CLEAN_RESID(64); break;
    }
#undef FCD_CLEAN_RESID
    FCD_LAUNCH_CHECK();
    if (Q > 0) {
        hipLaunchKernelGGL(clean_finish_kernel, dim3((unsigned)((S * Nreg + 3) / 4)), dim3(256), 0, st, nk, ss, flag, sflag, S * Nreg,
                           (int)Nreg, (int)Q, (int)T, resid);
        FCD_LAUNCH_CHECK();
    }
    return FCD_OK;
}
