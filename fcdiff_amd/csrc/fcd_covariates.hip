// K_cov: per-connection adjustment for subject covariates, fitted on the controls (fcd_edge_cov_fit, fcd_edge_cov_apply).
//
// Fit, per connection c over the controls observed at c (all of them without FCD_DATA_NAN_MISSING), the rules of K_clean:
//   1. every column of z is centred by its mean over the observed controls (the implied intercept);
//   2. a column constant over them (min == max) is dropped; the others are scaled to unit norm, so that the pivoting below
//      starts from remaining squared norms of exactly 1;
//   3. collinear columns are dropped by diagonally pivoted Cholesky of the Gram matrix (remaining squared norm below 1e-10:
//      not used; ties go to the lowest column index); rank = columns used, dof = n_obs - 1 - rank;
//   4. beta from the normal equations of the used columns, in the units of the original columns, 0 for a dropped column;
//   5. resid_var = (sum of squares of the residuals themselves) / dof;
//   6. dof < 1: nothing is fitted (beta row 0, rank 0, mask 0, resid_var NaN).
//
// Kernels (caller's stream, fixed reduction orders, no atomics: two calls agree bit for bit):
//   cov_design_kernel  one wave: steps 1-3 for the design of ALL controls, which every connection with a complete row shares.
//                      Leaves in the workspace ZS (H, 16), the centred unit-norm design, and Wt (H, 16) = ZS G^-1, so that
//                      the scaled beta of a complete row is the skinny product Wt^T (y - mean y).
//   cov_fit_kernel     one wave per connection, four to a workgroup, no workgroup barrier (the waves of a workgroup take
//                      different paths).  The row is read once from memory and again from cache.
//                        complete row:  beta = Wt^T (y - mean y) in plain fp64 multiply-adds: lane l takes column l & 15 of
//                                       every fourth control (64 consecutive doubles of Wt per step), two shuffles;
//                        row with NaN:  its own design: sums / min / max per column, then ONE MFMA pass that gives the Gram
//                                       matrix (A = B = the centred value, 0 at a missing control) and Z^T y, the Cholesky
//                                       and the substitutions in the wave's 2.8 KiB of LDS.  No lane holds a private Gram.
//                      Then the residuals of the row, lanes over the controls.
//   cov_apply_kernel   out = x - sum_q beta[c,q] (z[s,q] - z_ref[q]), q ascending from 0.0, one multiply and one add per
//                      term (no contraction): a workgroup stages z - z_ref of 256 columns once and walks 32 rows with it,
//                      16 bytes per lane where the shape allows.
#include "fcd_common.h"

#include <float.h>

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int CQ = 16;                   // covariate columns (one MFMA tile; the bit mask of info)
constexpr int CLD = CQ + 1;              // padded row of the wave's Gram matrix
constexpr double DROP_TOL = 1e-10;       // remaining squared norm of a unit-norm column below which it is not used

// What one wave owns in LDS.  A: Gram matrix of the unit-norm columns, then its pivoted Cholesky factor in place, in
// clean_chol_kernel's convention: L[piv[k]][m] = A[piv[k]][piv[m]], m <= k.
struct cov_wave {
    double A[CQ * CLD];
    double c[CQ];        // Z^T y of the unit-norm columns, by column
    double cs[CQ];       // ... in pivot order: becomes the solution of the normal equations
    double mean[CQ];
    double scale[CQ];    // 1 / norm of the centred column; 0: constant
    double bu[CQ];       // coefficient by column as the residual pass takes it; 0: not used
    int piv[CQ];
    int taken[CQ];
};

// Orders the wave's LDS traffic: what the lanes wrote before is what they read after.
__device__ __forceinline__ void cov_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double cov_readlane(double v, int j) {      // lane j's value, wave-uniform (j a constant)
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, j);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), j);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ double cov_sum_rows(double v) {      // over the four lanes that share l & 15
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// Steps 1-3 for the controls h with y[h] observed (y == nullptr or !missing: all), and Z^T (y - ybar) beside the Gram matrix.
// In the MFMA passes lane l holds column q = l & 15 of control h0 + (l >> 4).  Leaves w.A (factor), w.c, w.mean, w.scale,
// w.piv; returns rank and the mask of the columns used.
__device__ void cov_wave_design(cov_wave &w, const double *__restrict__ z, const double *__restrict__ y, bool missing, int H,
                                int Q, int n_obs, double ybar, int lane, int &rank_out, int &mask_out) {
    const int q = lane & 15, hs = lane >> 4;
    const bool col = q < Q;
    double sum = 0.0, mn = DBL_MAX, mx = -DBL_MAX;
#pragma unroll 4
    for (int h0 = 0; h0 < H; h0 += 4) {
        const int h = h0 + hs;
        bool ob = h < H && col;
        if (ob && missing) {
            const double yv = y[h];
            ob = yv == yv;
        }
        if (ob) {
            const double v = z[(int64_t)h * Q + q];
            sum += v;
            mn = fmin(mn, v);
            mx = fmax(mx, v);
        }
    }
    sum = cov_sum_rows(sum);
    mn = fmin(mn, __shfl_xor(mn, 16, 64));
    mn = fmin(mn, __shfl_xor(mn, 32, 64));
    mx = fmax(mx, __shfl_xor(mx, 16, 64));
    mx = fmax(mx, __shfl_xor(mx, 32, 64));
    const double mu = sum / (double)n_obs;
    const bool live = col && mn != mx;                       // (n_obs >= 1 here)
    double4_t g = double4_t{0.0, 0.0, 0.0, 0.0}, gy = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int h0 = 0; h0 < H; h0 += 4) {
        const int h = h0 + hs;
        double v = 0.0, yc = 0.0;
        if (h < H) {
            const double yv = y ? y[h] : 0.0;
            if (!missing || yv == yv) {
                yc = yv - ybar;
                if (live) v = z[(int64_t)h * Q + q] - mu;
            }
        }
        g = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, g, 0, 0, 0);
        gy = __builtin_amdgcn_mfma_f64_16x16x4f64(v, yc, gy, 0, 0, 0);
    }
    // result element r of lane l: row hs + 4 r, column q
#pragma unroll
    for (int r = 0; r < 4; ++r) w.A[(hs + 4 * r) * CLD + q] = g[r];
    if (q == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) w.c[hs + 4 * r] = gy[r];
    }
    cov_wave_sync();
    if (lane < CQ) {
        const double d = w.A[lane * CLD + lane];
        double sc = (lane < Q && mn != mx) ? 1.0 / sqrt(d) : 0.0;
        if (!(sc <= DBL_MAX)) sc = 0.0;
        w.scale[lane] = sc;
        w.mean[lane] = lane < Q ? mu : 0.0;
        w.taken[lane] = 0;
        w.bu[lane] = 0.0;
    }
    cov_wave_sync();
    for (int e = lane; e < CQ * CQ; e += 64) {
        const int i = e >> 4, j = e & 15;
        const double si = w.scale[i], sj = w.scale[j];
        w.A[i * CLD + j] = i == j ? (si != 0.0 ? 1.0 : 0.0) : w.A[i * CLD + j] * si * sj;
    }
    if (lane < CQ) w.c[lane] = w.c[lane] * w.scale[lane];
    cov_wave_sync();
    int rank = 0, mask = 0;
    for (int k = 0; k < Q; ++k) {
        double d = (lane < Q && !w.taken[lane]) ? w.A[lane * CLD + lane] : -1.0;
        if (!(d == d)) d = -1.0;
        int i = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(d, o, 64);
            const int oi = __shfl_xor(i, o, 64);
            if (od > d || (od == d && oi < i)) {
                d = od;
                i = oi;
            }
        }
        const int p = i;
        if (!(d >= DROP_TOL)) break;                          // (uniform)
        const double lpp = sqrt(d);
        if (lane < Q && !w.taken[lane] && lane != p) w.A[lane * CLD + p] = w.A[lane * CLD + p] / lpp;
        cov_wave_sync();
        for (int e = lane; e < Q * Q; e += 64) {
            const int a = e / Q, b = e % Q;
            if (a != p && b != p && !w.taken[a] && !w.taken[b]) w.A[a * CLD + b] -= w.A[a * CLD + p] * w.A[b * CLD + p];
        }
        cov_wave_sync();
        if (lane == 0) {
            w.A[p * CLD + p] = lpp;
            w.taken[p] = 1;
            w.piv[k] = p;
        }
        ++rank;
        mask |= 1 << p;
        cov_wave_sync();
    }
    rank_out = rank;
    mask_out = mask;
}

// Normal equations of the used columns by forward and back substitution on w.cs, one column of the factor per step; then
// w.bu[column] = coefficient on the centred, UNscaled column.
__device__ void cov_wave_solve(cov_wave &w, int rank, int lane) {
    if (lane < rank) w.cs[lane] = w.c[w.piv[lane]];
    cov_wave_sync();
    for (int k = 0; k < rank; ++k) {
        const int pk = w.piv[k];
        const double yk = w.cs[k] / w.A[pk * CLD + pk];
        cov_wave_sync();
        if (lane > k && lane < rank) w.cs[lane] -= w.A[w.piv[lane] * CLD + pk] * yk;
        if (lane == k) w.cs[k] = yk;
        cov_wave_sync();
    }
    for (int k = rank - 1; k >= 0; --k) {
        const int pk = w.piv[k];
        const double xk = w.cs[k] / w.A[pk * CLD + pk];
        cov_wave_sync();
        if (lane < k) w.cs[lane] -= w.A[pk * CLD + w.piv[lane]] * xk;
        if (lane == k) w.cs[k] = xk;
        cov_wave_sync();
    }
    if (lane < rank) {
        const int p = w.piv[lane];
        w.bu[p] = w.cs[lane] * w.scale[p];
    }
    cov_wave_sync();
}

// workspace of one fit call: ZS (H, 16) | Wt (H, 16) | scale (16) | {rank, mask} of the all-controls design
struct cov_ws {
    double *ZS, *Wt, *scale;
    int *hdr;
};
__host__ __device__ static inline cov_ws cov_ws_at(void *ws, int64_t H) {
    cov_ws o;
    o.ZS = (double *)ws;
    o.Wt = o.ZS + H * CQ;
    o.scale = o.Wt + H * CQ;
    o.hdr = (int *)(o.scale + CQ);
    return o;
}

__global__ __launch_bounds__(64) void cov_design_kernel(const double *__restrict__ z, int H, int Q, cov_ws ws) {
    __shared__ cov_wave w;
    __shared__ double Lp[CQ * CQ];       // the factor in pivot order: Lp[k][m] = L[piv[k]][piv[m]], m <= k
    const int lane = threadIdx.x;
    int rank = 0, mask = 0;
    cov_wave_design(w, z, nullptr, false, H, Q, H, 0.0, lane, rank, mask);
    for (int e = lane; e < rank * rank; e += 64) {
        const int k = e / rank, m = e % rank;
        Lp[k * CQ + m] = w.A[w.piv[k] * CLD + w.piv[m]];
    }
    cov_wave_sync();
    for (int h = lane; h < H; h += 64) {
        double v[CQ];
#pragma unroll
        for (int k = 0; k < CQ; ++k) {
            double x = 0.0;
            if (k < Q) x = (z[(int64_t)h * Q + k] - w.mean[k]) * w.scale[k];
            ws.ZS[(int64_t)h * CQ + k] = x;
            ws.Wt[(int64_t)h * CQ + k] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < CQ; ++k) {
            v[k] = 0.0;
            if (k < rank) {
                const int p = w.piv[k];
                v[k] = (z[(int64_t)h * Q + p] - w.mean[p]) * w.scale[p];
            }
        }
#pragma unroll
        for (int k = 0; k < CQ; ++k) {
            if (k < rank) {
                double t = v[k];
#pragma unroll
                for (int m = 0; m < k; ++m) t -= Lp[k * CQ + m] * v[m];
                v[k] = t / Lp[k * CQ + k];
            }
        }
#pragma unroll
        for (int k = CQ - 1; k >= 0; --k) {
            if (k < rank) {
                double t = v[k];
#pragma unroll
                for (int m = k + 1; m < CQ; ++m)
                    if (m < rank) t -= Lp[m * CQ + k] * v[m];
                v[k] = t / Lp[k * CQ + k];
            }
        }
#pragma unroll
        for (int k = 0; k < CQ; ++k)
            if (k < rank) ws.Wt[(int64_t)h * CQ + w.piv[k]] = v[k];
    }
    if (lane < CQ) ws.scale[lane] = w.scale[lane];
    if (lane == 0) {
        ws.hdr[0] = rank;
        ws.hdr[1] = mask;
    }
}

constexpr int FIT_WAVES = 4;
__global__ __launch_bounds__(64 * FIT_WAVES) void cov_fit_kernel(const double *__restrict__ b, const double *__restrict__ z,
                                                                 int64_t C, int H, int Q, int missing, cov_ws ws,
                                                                 double *__restrict__ beta, double *__restrict__ resid_var,
                                                                 int *__restrict__ info) {
    __shared__ cov_wave lds[FIT_WAVES];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t c = (int64_t)blockIdx.x * FIT_WAVES + wv;
    if (c >= C) return;
    cov_wave &w = lds[wv];
    const double *__restrict__ y = b + c * H;
    // the row once: how many controls are observed, their mean
    int n = 0;
    double sy = 0.0;
    for (int h = lane; h < H; h += 64) {
        const double yv = y[h];
        const bool ob = !missing || yv == yv;
        n += ob;
        if (ob) sy += yv;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    sy = fcd_wave_sum(sy);
    const int n_obs = n;
    const double ybar = sy / (double)n_obs;
    const bool complete = n_obs == H;
    int rank = 0, mask = 0;
    // wave-uniform, in registers: the coefficients as the residual pass takes them and what it subtracts from a column first
    double bu[CQ], mu[CQ];
#pragma unroll
    for (int q = 0; q < CQ; ++q) bu[q] = mu[q] = 0.0;
    bool shared = false;         // the residual pass reads ZS (coefficients in its units) instead of z
    if (n_obs >= 2 && Q > 0) {
        if (complete) {
            rank = ws.hdr[0];
            mask = ws.hdr[1];
            if (H - 1 - rank >= 1) {
                // Wt^T (y - ybar): lane l sums column l & 15 over the controls l >> 4, l >> 4 + 4, ... (64 consecutive
                // doubles of Wt per step), then over the four lanes of the column
                const int q = lane & 15, hs = lane >> 4;
                double acc = 0.0;
#pragma unroll 4
                for (int h = hs; h < H; h += 4) acc += ws.Wt[(int64_t)h * CQ + q] * (y[h] - ybar);
                acc = cov_sum_rows(acc);
#pragma unroll
                for (int k = 0; k < CQ; ++k) bu[k] = cov_readlane(acc, k);
                shared = true;
            }
        } else {
            cov_wave_design(w, z, y, true, H, Q, n_obs, ybar, lane, rank, mask);
            if (n_obs - 1 - rank >= 1) {
                cov_wave_solve(w, rank, lane);
#pragma unroll
                for (int k = 0; k < CQ; ++k) {
                    bu[k] = w.bu[k];
                    mu[k] = w.mean[k];
                }
            }
        }
    }
    const int dof = n_obs - 1 - rank;
    const bool fitted = dof >= 1;
    double rss = 0.0;
    if (fitted) {
        for (int h = lane; h < H; h += 64) {
            const double yv = y[h];
            double d = 0.0;
            if (rank > 0) {
                if (shared) {
                    const double2 *zr = reinterpret_cast<const double2 *>(ws.ZS + (int64_t)h * CQ);
#pragma unroll
                    for (int k = 0; k < CQ / 2; ++k) {
                        if (2 * k < Q) {                       // (columns beyond Q are zeros)
                            const double2 v = zr[k];
                            d += bu[2 * k] * v.x;
                            d += bu[2 * k + 1] * v.y;
                        }
                    }
                } else {
                    const double *zr = z + (int64_t)h * Q;
#pragma unroll
                    for (int q = 0; q < CQ; ++q)
                        if (q < Q) d += bu[q] * (zr[q] - mu[q]);
                }
            }
            const double r = (yv - ybar) - d;
            if (!missing || yv == yv) rss += r * r;
        }
        rss = fcd_wave_sum(rss);
    }
    if (lane < Q) {
        double bq = 0.0;
#pragma unroll
        for (int k = 0; k < CQ; ++k)
            if (lane == k) bq = bu[k];
        if (shared) bq = bq * ws.scale[lane];
        beta[c * Q + lane] = bq;
    }
    if (lane == 0) {
        resid_var[c] = fitted ? rss / (double)dof : __builtin_nan("");
        info[c * 4 + 0] = n_obs;
        info[c * 4 + 1] = fitted ? rank : 0;
        info[c * 4 + 2] = dof;
        info[c * 4 + 3] = fitted ? mask : 0;
    }
}

// grid = (blocks of AR rows, blocks of AS columns).  VEC: S is even and x / out are 16-byte aligned, a lane takes two columns.
constexpr int AR = 32, AS = 256;
template <bool VEC>
__global__ __launch_bounds__(256) void cov_apply_kernel(const double *__restrict__ x, const double *__restrict__ z,
                                                        const double *__restrict__ z_ref, const double *__restrict__ beta,
                                                        int64_t C, int64_t S, int Q, double *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) double zc[AS * CQ];      // [q][column]: z - z_ref of this block's columns
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.y * AS, c0 = (int64_t)blockIdx.x * AR;
    const int ns = (int)(S - s0 < AS ? S - s0 : AS);
    for (int e = tid; e < ns * Q; e += 256) {
        const int j = e / Q, q = e % Q;
        zc[q * AS + j] = z[(s0 + j) * Q + q] - z_ref[q];
    }
    __syncthreads();
    constexpr int W = VEC ? 2 : 1, TPR = AS / W, RPI = 256 / TPR;   // columns per lane, lanes per row, rows per iteration
    const int j = (tid % TPR) * W, rr = tid / TPR;
    if (j >= ns) return;
    for (int r = rr; r < AR; r += RPI) {
        const int64_t c = c0 + r;
        if (c >= C) break;
        const double *bq = beta + c * Q;
        double d[W];
#pragma unroll
        for (int t = 0; t < W; ++t) d[t] = 0.0;
        for (int q = 0; q < Q; ++q) {
            const double bv = bq[q];
#pragma unroll
            for (int t = 0; t < W; ++t) d[t] = d[t] + bv * zc[q * AS + j + t];
        }
        const int64_t at = c * S + s0 + j;
        if (VEC) {
            const double2 xv = *reinterpret_cast<const double2 *>(x + at);      // (ns is even: j + 1 < ns)
            *reinterpret_cast<double2 *>(out + at) = make_double2(xv.x - d[0], xv.y - d[W - 1]);
        } else {
            out[at] = x[at] - d[0];
        }
    }
}

}  // namespace

extern "C" int fcd_edge_cov_fit(fcd_ctx *ctx, const double *b, int64_t C, int64_t H, const double *z, int64_t Q, int flags,
                                double *beta, double *resid_var, int32_t *info, fcd_stream stream) {
    if (!ctx || !b || !resid_var || !info) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_edge_cov_fit: null pointer");
    if (flags & ~FCD_DATA_NAN_MISSING) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_edge_cov_fit: unknown flags 0x%llx", flags);
    if (C < 1 || H < 1) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_edge_cov_fit: C=%lld H=%lld must be >= 1", C, H);
    if (Q < 0) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_edge_cov_fit: Q=%lld is negative", Q);
    if (Q > CQ) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_edge_cov_fit: Q=%lld covariate columns, at most 16", Q);
    if (Q > 0 && (!z || !beta)) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_edge_cov_fit: Q=%lld but z or beta is null", Q);
    if (H > (1 << 26) || (C + FIT_WAVES - 1) / FIT_WAVES > INT32_MAX)
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_edge_cov_fit: shape too large (C=%lld, H=%lld)", C, H);
    hipStream_t st = (hipStream_t)stream;
    // Nothing of the workspace outlives the call.
    int rc = fcd_ws_reserve(ctx, (size_t)(2 * H * CQ + CQ) * sizeof(double) + 4 * sizeof(int));
    if (rc) return rc;
    const cov_ws ws = cov_ws_at(ctx->ws.p, H);
    if (Q > 0) {
        hipLaunchKernelGGL(cov_design_kernel, dim3(1), dim3(64), 0, st, z, (int)H, (int)Q, ws);
        FCD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cov_fit_kernel, dim3((unsigned)((C + FIT_WAVES - 1) / FIT_WAVES)), dim3(64 * FIT_WAVES), 0, st, b, z, C, (int)H,
                       (int)Q, (flags & FCD_DATA_NAN_MISSING) ? 1 : 0, ws, beta, resid_var, info);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_edge_cov_apply(fcd_ctx *ctx, const double *x, int64_t C, int64_t S, const double *z, int64_t Q,
                                  const double *z_ref, const double *beta, double *out, fcd_stream stream) {
    if (!ctx || !x || !out) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_edge_cov_apply: null pointer");
    if (C < 1 || S < 1) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_edge_cov_apply: C=%lld S=%lld must be >= 1", C, S);
    if (Q < 0) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_edge_cov_apply: Q=%lld is negative", Q);
    if (Q > CQ) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_edge_cov_apply: Q=%lld covariate columns, at most 16", Q);
    if (Q > 0 && (!z || !z_ref || !beta)) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_edge_cov_apply: Q=%lld but z, z_ref or beta is null", Q);
    const int64_t gx = (C + AR - 1) / AR, gy = (S + AS - 1) / AS;
    if (gx > INT32_MAX || gy > 65535) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_edge_cov_apply: shape too large (C=%lld, S=%lld)", C, S);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (S % 2 == 0) && (((uintptr_t)x | (uintptr_t)out) % 16 == 0);
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (vec)
        hipLaunchKernelGGL(cov_apply_kernel<true>, grid, dim3(256), 0, st, x, z, z_ref, beta, C, S, (int)Q, out);
    else
        hipLaunchKernelGGL(cov_apply_kernel<false>, grid, dim3(256), 0, st, x, z, z_ref, beta, C, S, (int)Q, out);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
