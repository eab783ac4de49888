// Repeated sessions per patient: the likelihood tables and the connection posterior for bt (C, U, K), K scans of each
// patient, session the fastest index.
//
// F~_cu is the patient's latent state of the connection and the K sessions are conditionally independent measurements of
// it, so the density of an item given F~ = j is the product over its sessions:
//   P_j(c,u)  = prod_k N(bt[c,u,k]; mu_j, sigma_j)                 (a NaN session contributes 1 under FCD_DATA_NAN_MISSING)
//   M_kl(c,u) = e_l P_k + (1 - e_l)/2 sum_{j != k} P_j             (e_l = _eval_M_eps, as in K_lik)
// A product of K densities underflows (sigma = 0.05, 16 sessions at 1.0: every P_j = 0 in fp64), so it is never formed:
//   a_j = sum_k ln N_j(x_k)  (lik_normal_logs, ascending k, fp64),  m = max_j a_j,  p_j = exp(a_j - m),
//   lM  = m + ln M_kl(p).
// One p_j is exactly 1, so every M_kl(p) >= cmin > 0 and the nine logs take lik_logs' branch-free form (its general log
// where eps is 0 or 1).  A NaN session adds exactly 0.0 to a_j: the table of K sessions with one of them NaN everywhere
// equals the table of the other K - 1 bit for bit.  An item with no observed session is stored as 0.0 by a select;
// m = -inf (every density of some session underflowed its log) gives -inf in all nine entries.
//
// Three kernels:
//   lik_sessions_kernel         K_lik's launch: item blocks (one thread per (c,u), results through the LDS transpose and
//                               non-temporal 16-byte stores) and K_lik's S_B blocks (lik_sb_block, so S_B and lp_B_g_F equal
//                               fcd_lik_tables_ex's bit for bit).  The K doubles of a tile's 256 items are one contiguous
//                               span of 256 K doubles: it is loaded coalesced through `stage` before the results overwrite
//                               it, at most 9 sessions per item and pass, so the kernel holds K_lik's LDS and no more.
//   lik_shared_sessions_kernel  K_lik_shared's launch with the session-summed item: L[c] = sum_u lM[c,u].
//   posterior_sessions_kernel   fcd_post.hip's posterior_kernel with a_j summed over the item's sessions; an item with no
//                               observed session gets the prior law.  (posterior_kernel keeps its own text, as lik_kernel
//                               does: the 2-D kernels are not changed by this file.)
#include "fcd_lik_common.h"

namespace {

constexpr int SESS_PASS = 9;      // sessions per item and pass: 256 x 9 doubles, the stage buffer of the results

// one session's three ln N_j into a[]; MISSING: a NaN session adds exactly 0.0 and is counted
template <bool MISSING>
__device__ __forceinline__ void sess_add(double x, const LikTheta &th, double a[3], int &n_obs, unsigned &n_nan) {
    double l0, l1, l2;
    lik_normal_logs(x, th, l0, l1, l2);
    if (MISSING) {
        const bool miss = __builtin_isnan(x);
        l0 = miss ? 0.0 : l0;
        l1 = miss ? 0.0 : l1;
        l2 = miss ? 0.0 : l2;
        n_nan += miss;
        n_obs += !miss;
    }
    a[0] += l0;
    a[1] += l1;
    a[2] += l2;
}

// v[k*3+l] = m + ln M_kl(exp(a - m)); `empty`: no observed session, exactly 0.0
__device__ __forceinline__ void sess_logs(const double a[3], bool empty, const LikTheta &th, const double *etab,
                                          const fcd_log_cell *ltab, double v[9]) {
    const double m = fmax(a[0], fmax(a[1], a[2]));
    double p[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = fcd_exp_neg(m - a[j], etab);       // one of them exactly 1; NaN stays NaN
    lik_logs(p, th, ltab, v);
    const bool dead = m == -__builtin_inf();                               // (a - m would be NaN)
#pragma unroll
    for (int j = 0; j < 9; ++j) v[j] = empty ? 0.0 : (dead ? -__builtin_inf() : m + v[j]);
}

template <bool MISSING>
__global__ __launch_bounds__(LIK_BLOCK) void lik_sessions_kernel(const double *__restrict__ bt, int64_t n_items, int K,
                                                                 LikTheta th, const LikTabs *__restrict__ tabs,
                                                                 double *__restrict__ lM, int n_bt_blocks,
                                                                 const double *__restrict__ b, int64_t C, int H,
                                                                 double *__restrict__ S_B, double *__restrict__ lpB,
                                                                 unsigned long long *__restrict__ nan_slots) {
    __shared__ __attribute__((aligned(16))) double stage[LIK_BLOCK * SESS_PASS];
    __shared__ __attribute__((aligned(16))) fcd_log_cell ltab[FCD_LOG_CELLS];
    __shared__ double etab[FCD_EXP_CELLS];
    __shared__ int blk_nan;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_bt_blocks) {
        lik_sb_block<MISSING>(blockIdx.x - n_bt_blocks, tid, b, C, H, th, S_B, lpB, nan_slots, &blk_nan);
        return;
    }
    for (int t = tid; t < FCD_LOG_CELLS; t += LIK_BLOCK) ltab[t] = tabs->log_tab[t];
    if (tid < FCD_EXP_CELLS) etab[tid] = tabs->exp_tab[tid];
    if (MISSING && tid == 0) blk_nan = 0;
    __syncthreads();
    unsigned n_nan = 0;
    const int64_t n_tiles = (n_items + LIK_BLOCK - 1) / LIK_BLOCK;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += n_bt_blocks) {
        const int64_t base = tile * LIK_BLOCK;
        const int n_here = (n_items - base < LIK_BLOCK) ? (int)(n_items - base) : LIK_BLOCK;
        double a[3] = {0.0, 0.0, 0.0};
        int n_obs = 0;
        for (int64_t k0 = 0; k0 < K; k0 += SESS_PASS) {
            const int P = (K - k0 < SESS_PASS) ? (int)(K - k0) : SESS_PASS;
#ifdef FCD_SESS_STRIDED
            // measurement build only (profiles/sessions_cost.py): every thread reads its own item's sessions, K doubles apart
            if (tid < n_here) {
                const double *x = bt + (base + tid) * K + k0;
                for (int s = 0; s < P; ++s) sess_add<MISSING>(x[s], th, a, n_obs, n_nan);
            }
#else
            const int n = n_here * P;                               // <= 256 * 9: the pass fits the stage buffer
            const double *src = bt + base * K + k0;                 // item q's sessions k0 .. k0 + P - 1 at src + q K
            if (P == K) {
                for (int j = tid; j < n; j += LIK_BLOCK) stage[j] = src[j];           // (rows of odd K are 8-byte aligned)
            } else {
                for (int j = tid; j < n; j += LIK_BLOCK) {
                    const int q = j / P;
                    stage[j] = src[(int64_t)q * K + (j - q * P)];
                }
            }
            __syncthreads();
            if (tid < n_here)
                for (int s = 0; s < P; ++s) sess_add<MISSING>(stage[tid * P + s], th, a, n_obs, n_nan);
            __syncthreads();                                        // the pass is read: the next one, or the results
#endif
        }
        if (tid < n_here) {
            double v[9];
            sess_logs(a, MISSING && n_obs == 0, th, etab, ltab, v);
#pragma unroll
            for (int j = 0; j < 9; ++j) stage[tid * 9 + j] = v[j];
        }
        __syncthreads();
        const int64_t n_dbl = (int64_t)n_here * 9;
        double *dst = lM + base * 9;
        // base*9*8 bytes is a multiple of 16 (LIK_BLOCK*72), so double2 stores are aligned; non-temporal as in lik_kernel
        const int64_t n_d2 = n_dbl >> 1;
        const double2 *s2 = reinterpret_cast<const double2 *>(stage);
        double2 *d2 = reinterpret_cast<double2 *>(dst);
        {
            typedef double d2v __attribute__((ext_vector_type(2)));
            for (int64_t j = tid; j < n_d2; j += LIK_BLOCK)
                __builtin_nontemporal_store(*reinterpret_cast<const d2v *>(&s2[j]), reinterpret_cast<d2v *>(&d2[j]));
        }
        if ((n_dbl & 1) && tid == 0) dst[n_dbl - 1] = stage[n_dbl - 1];
        __syncthreads();
    }
    if (MISSING) {
        if (n_nan) atomicAdd(&blk_nan, (int)n_nan);
        __syncthreads();
        if (tid == 0 && blk_nan && nan_slots)
            atomicAdd(&nan_slots[(blockIdx.x % FCD_NAN_SLOTS) * 16 + 1], (unsigned long long)blk_nan);
    }
}

template <bool MISSING, int G>
__global__ __launch_bounds__(LIK_BLOCK) void lik_shared_sessions_kernel(const double *__restrict__ bt, int64_t C, int U, int K,
                                                                        LikTheta th, const LikTabs *__restrict__ tabs,
                                                                        double *__restrict__ L, int n_l_blocks,
                                                                        const double *__restrict__ b, int H,
                                                                        double *__restrict__ S_B,
                                                                        unsigned long long *__restrict__ nan_slots) {
    static_assert(G == 16 || G == 32 || G == 64, "lane group of 16, 32 or 64");
    __shared__ __attribute__((aligned(16))) fcd_log_cell ltab[FCD_LOG_CELLS];
    __shared__ double etab[FCD_EXP_CELLS];
    __shared__ int blk_nan;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_l_blocks) {
        lik_sb_block<MISSING>(blockIdx.x - n_l_blocks, tid, b, C, H, th, S_B, nullptr, nan_slots, &blk_nan);
        return;
    }
    for (int t = tid; t < FCD_LOG_CELLS; t += LIK_BLOCK) ltab[t] = tabs->log_tab[t];
    if (tid < FCD_EXP_CELLS) etab[tid] = tabs->exp_tab[tid];
    if (MISSING && tid == 0) blk_nan = 0;
    __syncthreads();
    constexpr int EPB = LIK_BLOCK / G;          // edges per block and pass
    const int lane = tid & (G - 1);
    unsigned n_nan = 0;
    for (int64_t c0 = (int64_t)blockIdx.x * EPB; c0 < C; c0 += (int64_t)n_l_blocks * EPB) {
        const int64_t c = c0 + tid / G;         // the same for the G lanes of a group
        double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (c < C) {
            for (int u = lane; u < U; u += G) {
                const double *x = bt + (c * U + u) * K;             // the item's K sessions
                double a[3] = {0.0, 0.0, 0.0}, v[9];
                int n_obs = 0;
                for (int k = 0; k < K; ++k) sess_add<MISSING>(x[k], th, a, n_obs, n_nan);
                sess_logs(a, MISSING && n_obs == 0, th, etab, ltab, v);
#pragma unroll
                for (int j = 0; j < 9; ++j) s[j] += v[j];
            }
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1)
#pragma unroll
            for (int j = 0; j < 9; ++j) s[j] += __shfl_xor(s[j], o, G);
        if (c < C && lane == 0) {
#pragma unroll
            for (int j = 0; j < 9; ++j) L[c * 9 + j] = s[j];
        }
    }
    if (MISSING) {
        __syncthreads();
        if (n_nan) atomicAdd(&blk_nan, (int)n_nan);
        __syncthreads();
        if (tid == 0 && blk_nan && nan_slots)
            atomicAdd(&nan_slots[(blockIdx.x % FCD_NAN_SLOTS) * 16 + 1], (unsigned long long)blk_nan);
    }
}

template <bool MISSING>
void lik_shared_sessions_launch(int group, dim3 grid, hipStream_t s, const double *bt, int64_t C, int U, int K, const LikTheta &th,
                                const LikTabs *tabs, double *L, int n_l_blocks, const double *b, int H, double *S_B,
                                unsigned long long *slots) {
    if (group == 16)
        hipLaunchKernelGGL((lik_shared_sessions_kernel<MISSING, 16>), grid, dim3(LIK_BLOCK), 0, s, bt, C, U, K, th, tabs, L,
                           n_l_blocks, b, H, S_B, slots);
    else if (group == 32)
        hipLaunchKernelGGL((lik_shared_sessions_kernel<MISSING, 32>), grid, dim3(LIK_BLOCK), 0, s, bt, C, U, K, th, tabs, L,
                           n_l_blocks, b, H, S_B, slots);
    else
        hipLaunchKernelGGL((lik_shared_sessions_kernel<MISSING, 64>), grid, dim3(LIK_BLOCK), 0, s, bt, C, U, K, th, tabs, L,
                           n_l_blocks, b, H, S_B, slots);
}

struct SessPostTheta {
    double mu[3], sigma[3], lsigma[3];
    double eps;           // epsilon
    double e[3];          // _eval_M_eps(eta, epsilon, l)
    double pT[3];         // p(T = 1 | l) = 0, 1, eta
};

// posterior_kernel (fcd_post.hip) statement for statement, except that a_j is summed over the item's K sessions before the
// maximum is taken.  MISSING: a NaN session is skipped; an item with no observed session takes N_j = 1, the prior law.
template <bool MISSING>
__global__ __launch_bounds__(256) void posterior_sessions_kernel(const double *__restrict__ bt, int64_t C, int U, int K,
                                                                 SessPostTheta th, const uint32_t *__restrict__ counts,
                                                                 const double *__restrict__ lq_F, const double *__restrict__ lq_R,
                                                                 double *__restrict__ p_T, double *__restrict__ p_Ft,
                                                                 double *__restrict__ p_ch) {
    const int64_t items = C * U;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        double W[9];
        if (counts) {
            const uint32_t *cw = counts + i * 9;
#pragma unroll
            for (int j = 0; j < 9; ++j) W[j] = (double)cw[j];
        } else {
            const int64_t c = i / U;
            const int u = (int)(i - c * U);
            int n, m;
            fcd_edge_to_pair(c, n, m);
            const double q0n = exp(lq_R[((int64_t)n * U + u) * 2]), q1n = exp(lq_R[((int64_t)n * U + u) * 2 + 1]);
            const double q0m = exp(lq_R[((int64_t)m * U + u) * 2]), q1m = exp(lq_R[((int64_t)m * U + u) * 2 + 1]);
            double w[3];
            w[0] = q0n * q0m;
            w[1] = q1n * q1m;
            w[2] = q0n * q1m;
            w[2] += q1n * q0m;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double qF = exp(lq_F[c * 3 + k]);
#pragma unroll
                for (int l = 0; l < 3; ++l) W[k * 3 + l] = qF * w[l];
            }
        }
        const double *x = bt + i * K;
        double a[3] = {0.0, 0.0, 0.0};
        int n_obs = 0;
        for (int k = 0; k < K; ++k) {
            const double xk = x[k];
            if (MISSING && __builtin_isnan(xk)) continue;          // unobserved: the session's densities integrate to 1
            ++n_obs;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double z = (xk - th.mu[j]) / th.sigma[j];
                a[j] += -(z * z) / 2.0 - th.lsigma[j];               // ln N_j up to the common ln sqrt(2 pi)
            }
        }
        double N[3];
        if (MISSING && n_obs == 0) {
            N[0] = N[1] = N[2] = 1.0;
        } else {
            const double mx = fmax(a[0], fmax(a[1], a[2]));
#pragma unroll
            for (int j = 0; j < 3; ++j) N[j] = exp(a[j] - mx);
        }
        const double S[3] = {N[1] + N[2], N[0] + N[2], N[0] + N[1]};
        double wsum = 0.0, t1 = 0.0, ch = 0.0, ft[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                const double wt = W[k * 3 + l];
                if (wt == 0.0) continue;
                const double off = (1 - th.e[l]) * 0.5;
                const double M = th.e[l] * N[k] + off * S[k];
                if (!(M > 0.0)) continue;                    // (only at epsilon in {0, 1}: a case the model gives no mass)
                const double r = wt / M;
                wsum += wt;
                if (th.pT[l] != 0.0) t1 += th.pT[l] * (th.eps * N[k] + (1 - th.eps) * 0.5 * S[k]) * r;
                ch += off * S[k] * r;
#pragma unroll
                for (int j = 0; j < 3; ++j) ft[j] += ((j == k) ? th.e[l] : off) * N[j] * r;
            }
        }
        const double inv = 1.0 / wsum;
        p_T[i] = t1 * inv;
        p_ch[i] = ch * inv;
#pragma unroll
        for (int j = 0; j < 3; ++j) p_Ft[i * 3 + j] = ft[j] * inv;
    }
}

// the checks the three entry points share with their 2-D siblings
int sessions_check(fcd_ctx *ctx, int64_t C, int64_t H, int64_t U, int64_t K, int flags, bool counted) {
    if (flags & ~FCD_DATA_NAN_MISSING) return fcd_fail(ctx, FCD_ERR_ARG, "sessions tables: unknown flags 0x%x", flags);
    if (counted && !(flags & FCD_DATA_NAN_MISSING))
        return fcd_fail(ctx, FCD_ERR_ARG, "sessions tables: missing counts need FCD_DATA_NAN_MISSING");
    if (C < 1 || H < 1 || U < 1) return fcd_fail(ctx, FCD_ERR_ARG, "sessions tables: C=%lld and U=%lld (and H) must be >= 1", C, U);
    if (K < 1) return fcd_fail(ctx, FCD_ERR_ARG, "sessions tables: K=%lld sessions, must be >= 1", K);
    if (fcd_C_to_N(C) < 0) return fcd_fail(ctx, FCD_ERR_SHAPE, "Number of connections (%lld) must be a triangular number.", C);
    if (H > INT32_MAX || U > INT32_MAX || K > INT32_MAX || C * U > INT64_MAX / 8 / K)
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "sessions tables: H/U/K too large");
    return FCD_OK;
}

}  // namespace

extern "C" int fcd_lik_tables_sessions(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U, int64_t K,
                                       const double *theta, double *S_B, double *lM, double *lp_B_g_F, int flags,
                                       int64_t *n_missing2, fcd_stream stream) {
    if (!ctx || !b || !bt || !theta || !S_B || !lM) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_tables_sessions: null pointer");
    int rc = sessions_check(ctx, C, H, U, K, flags, n_missing2 != nullptr);
    if (rc) return rc;
    LikTheta th;
    lik_theta_make(theta, th);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_items = C * U;
    const int64_t n_tiles = (n_items + LIK_BLOCK - 1) / LIK_BLOCK;
    int64_t grid = n_tiles;                          // K_lik's measured choice: 16 blocks per CU, grid-stride beyond
    const int64_t cap = (int64_t)ctx->num_cu * 16;
    if (grid > cap) grid = cap;
    const int64_t n_b_blocks = (C + 15) / 16;
    unsigned long long *slots = n_missing2 ? reinterpret_cast<unsigned long long *>(ctx->nan_slots) : nullptr;
    const LikTabs *tabs = reinterpret_cast<const LikTabs *>(ctx->log_tab);
    if (flags & FCD_DATA_NAN_MISSING)
        hipLaunchKernelGGL(lik_sessions_kernel<true>, dim3((unsigned)(grid + n_b_blocks)), dim3(LIK_BLOCK), 0, s, bt, n_items,
                           (int)K, th, tabs, lM, (int)grid, b, C, (int)H, S_B, lp_B_g_F, slots);
    else
        hipLaunchKernelGGL(lik_sessions_kernel<false>, dim3((unsigned)(grid + n_b_blocks)), dim3(LIK_BLOCK), 0, s, bt, n_items,
                           (int)K, th, tabs, lM, (int)grid, b, C, (int)H, S_B, lp_B_g_F, nullptr);
    FCD_LAUNCH_CHECK();
    if (slots) {
        hipLaunchKernelGGL(nan_fold_kernel, dim3(1), dim3(FCD_NAN_SLOTS), 0, s, slots, n_missing2);
        FCD_LAUNCH_CHECK();
    }
    return FCD_OK;
}

extern "C" int fcd_lik_shared_tables_sessions(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                              int64_t K, const double *theta, double *S_B, double *L, int flags,
                                              int64_t *nan_counts, fcd_stream stream) {
    if (!ctx || !b || !bt || !theta || !S_B || !L) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_shared_tables_sessions: null pointer");
    int rc = sessions_check(ctx, C, H, U, K, flags, nan_counts != nullptr);
    if (rc) return rc;
    LikTheta th;
    lik_theta_make(theta, th);
    hipStream_t s = (hipStream_t)stream;
    const int group = U <= 16 ? 16 : (U <= 32 ? 32 : 64);
    const int64_t epb = LIK_BLOCK / group;
    int64_t n_l = (C + epb - 1) / epb;               // one pass per block up to 16 blocks per CU, grid-stride beyond
    const int64_t cap = (int64_t)ctx->num_cu * 16;
    if (n_l > cap) n_l = cap;
    const int64_t n_b_blocks = (C + 15) / 16;
    const dim3 grid((unsigned)(n_l + n_b_blocks));
    unsigned long long *slots = nan_counts ? reinterpret_cast<unsigned long long *>(ctx->nan_slots) : nullptr;
    const LikTabs *tabs = reinterpret_cast<const LikTabs *>(ctx->log_tab);
    if (flags & FCD_DATA_NAN_MISSING)
        lik_shared_sessions_launch<true>(group, grid, s, bt, C, (int)U, (int)K, th, tabs, L, (int)n_l, b, (int)H, S_B, slots);
    else
        lik_shared_sessions_launch<false>(group, grid, s, bt, C, (int)U, (int)K, th, tabs, L, (int)n_l, b, (int)H, S_B, nullptr);
    FCD_LAUNCH_CHECK();
    if (slots) {
        hipLaunchKernelGGL(nan_fold_kernel, dim3(1), dim3(FCD_NAN_SLOTS), 0, s, slots, nan_counts);
        FCD_LAUNCH_CHECK();
    }
    return FCD_OK;
}

extern "C" int fcd_conn_posterior_sessions(fcd_ctx *ctx, const double *bt, int64_t Nreg, int64_t U, int64_t K, const double *theta,
                                           const uint32_t *counts, const double *lq_F, const double *lq_R, int flags, double *p_T,
                                           double *p_F_tilde, double *p_changed, fcd_stream stream) {
    if (!ctx || !bt || !theta || !p_T || !p_F_tilde || !p_changed)
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_conn_posterior_sessions: null pointer");
    if (flags & ~FCD_DATA_NAN_MISSING) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_conn_posterior_sessions: unknown flags 0x%x", flags);
    if ((counts != nullptr) == (lq_F != nullptr || lq_R != nullptr) || (!counts && (!lq_F || !lq_R)))
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_conn_posterior_sessions: pass counts, or lq_F and lq_R");
    if (Nreg < 2 || U < 1 || U > INT32_MAX || Nreg > 46340)
        return fcd_fail(ctx, FCD_ERR_SHAPE, "fcd_conn_posterior_sessions: Nreg=%lld U=%lld", Nreg, U);
    if (K < 1) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_conn_posterior_sessions: K=%lld sessions, must be >= 1", K);
    const int64_t C = fcd_tri(Nreg);
    if (K > INT32_MAX || C * U > INT64_MAX / 8 / K)
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_conn_posterior_sessions: K=%lld too large", K);
    SessPostTheta th;
    const double eta = theta[1], epsilon = theta[2];
    for (int k = 0; k < 3; ++k) {
        th.mu[k] = theta[6 + k];
        th.sigma[k] = theta[9 + k];
        th.lsigma[k] = log(th.sigma[k]);
        if (!(th.sigma[k] > 0.0)) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_conn_posterior_sessions: sigma must be > 0");
    }
    th.eps = epsilon;
    th.e[0] = 1 - epsilon;                        // _eval_M_eps, fit.py:433-444
    th.e[1] = epsilon;
    double e2 = eta * epsilon;
    e2 += (1 - eta) * (1 - epsilon);
    th.e[2] = e2;
    th.pT[0] = 0.0;
    th.pT[1] = 1.0;
    th.pT[2] = eta;
    const int64_t items = C * U;
    int64_t blocks = (items + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cu * 64;
    if (blocks > cap) blocks = cap;
    if (flags & FCD_DATA_NAN_MISSING)
        hipLaunchKernelGGL(posterior_sessions_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bt, C, (int)U,
                           (int)K, th, counts, lq_F, lq_R, p_T, p_F_tilde, p_changed);
    else
        hipLaunchKernelGGL(posterior_sessions_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bt, C,
                           (int)U, (int)K, th, counts, lq_F, lq_R, p_T, p_F_tilde, p_changed);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
