// K_lik_shared: the likelihood tables of the shared-region model (fcdiff_amd.fit.SharedRegionFit).
//
// With one set of anomalous regions for all patients the collapsed joint needs lM only through its patient sum
//   L[c,k,l] = sum_u lM[c,u,k,l] = sum_u ln M_kl(bt_cu),
// the table of the unshared model at ONE patient.  This launch reads b (C,H) and bt (C,U) once and writes S_B (C,3) and
// L (C,3,3); nothing of size C*U is ever written.  Algorithmic bytes per call = 8*C*(H+U) + 24*C + 72*C.
//
// One launch, two kinds of blocks (as K_lik):
// Blocks [0, n_l_blocks): a group of G lanes per edge (G = 16, 32 or 64 by U), grid-stride over edges.  Each lane takes
//   u = lane, lane + G, ... of the contiguous row bt[c, :], computes the nine ln M_kl of K_lik's per-item arithmetic
//   (fcd_lik_common.h: the fcd_fastmath.h tables in LDS, the cmin test, ocml's log at the edge of the double range) and
//   keeps nine running sums; a butterfly of shuffles within the group sums the lanes, and lane 0 writes the edge's
//   72-byte record.  No atomics in the sums: the order is fixed, so two calls agree bit for bit.
// Blocks [n_l_blocks, ...): the S_B blocks of K_lik (lik_sb_block), so S_B equals fcd_lik_tables' S_B bit for bit.
//
// MISSING (FCD_DATA_NAN_MISSING): a NaN bt adds 0 to L (its M_kl = 1), a NaN b adds 0 to S_B; the NaN counts go to the
// context's slot lines as in K_lik (word 0: b, word 1: bt) and nan_fold_kernel writes them.  Without the flag a NaN
// gives NaN, as lM would.  An item whose density underflows gives -inf, and so does the edge's sum.
#include "fcd_lik_common.h"

namespace {

template <bool MISSING, int G>
__global__ __launch_bounds__(LIK_BLOCK) void lik_shared_kernel(const double *__restrict__ bt, int64_t C, int U, LikTheta th,
                                                               const LikTabs *__restrict__ tabs, double *__restrict__ L,
                                                               int n_l_blocks, const double *__restrict__ b, int H,
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
    int nan_bt = 0;
    for (int64_t c0 = (int64_t)blockIdx.x * EPB; c0 < C; c0 += (int64_t)n_l_blocks * EPB) {
        const int64_t c = c0 + tid / G;         // the same for the G lanes of a group
        double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (c < C) {
            const double *row = bt + c * U;
            for (int u = lane; u < U; u += G) {
                double x = row[u];
                bool miss = false;
                if (MISSING) {
                    miss = __builtin_isnan(x);          // unobserved: M_kl = 1, adds 0 (a finite stand-in, then selects)
                    x = miss ? th.mu[0] : x;
                    nan_bt += miss;
                }
                double N[3], v[9];
                lik_densities(x, th, etab, N);          // fit.py:115
                lik_logs(N, th, ltab, v);               // fit.py:122, :430
#pragma unroll
                for (int j = 0; j < 9; ++j) s[j] += miss ? 0.0 : v[j];
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
        if (nan_bt) atomicAdd(&blk_nan, nan_bt);
        __syncthreads();
        if (tid == 0 && blk_nan && nan_slots)
            atomicAdd(&nan_slots[(blockIdx.x % FCD_NAN_SLOTS) * 16 + 1], (unsigned long long)blk_nan);
    }
}

template <bool MISSING>
void lik_shared_launch(int group, dim3 grid, hipStream_t s, const double *bt, int64_t C, int U, const LikTheta &th,
                       const LikTabs *tabs, double *L, int n_l_blocks, const double *b, int H, double *S_B,
                       unsigned long long *slots) {
    if (group == 16)
        hipLaunchKernelGGL((lik_shared_kernel<MISSING, 16>), grid, dim3(LIK_BLOCK), 0, s, bt, C, U, th, tabs, L, n_l_blocks, b,
                           H, S_B, slots);
    else if (group == 32)
        hipLaunchKernelGGL((lik_shared_kernel<MISSING, 32>), grid, dim3(LIK_BLOCK), 0, s, bt, C, U, th, tabs, L, n_l_blocks, b,
                           H, S_B, slots);
    else
        hipLaunchKernelGGL((lik_shared_kernel<MISSING, 64>), grid, dim3(LIK_BLOCK), 0, s, bt, C, U, th, tabs, L, n_l_blocks, b,
                           H, S_B, slots);
}

}  // namespace

extern "C" int fcd_lik_shared_tables(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                     const double *theta, double *S_B, double *L, int flags, int64_t *nan_counts,
                                     fcd_stream stream) {
    if (!ctx || !b || !bt || !theta || !S_B || !L) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_shared_tables: null pointer");
    if (flags & ~FCD_DATA_NAN_MISSING) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_shared_tables: unknown flags 0x%x", flags);
    const bool missing = (flags & FCD_DATA_NAN_MISSING) != 0;
    if (nan_counts && !missing)
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_shared_tables: missing counts need FCD_DATA_NAN_MISSING");
    if (C < 1 || H < 1 || U < 1)
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_shared_tables: C=%lld and U=%lld (and H) must be >= 1", C, U);
    if (fcd_C_to_N(C) < 0) return fcd_fail(ctx, FCD_ERR_SHAPE, "Number of connections (%lld) must be a triangular number.", C);
    if (H > INT32_MAX || U > INT32_MAX) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_lik_shared_tables: H/U too large");
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
    if (missing)
        lik_shared_launch<true>(group, grid, s, bt, C, (int)U, th, tabs, L, (int)n_l, b, (int)H, S_B, slots);
    else
        lik_shared_launch<false>(group, grid, s, bt, C, (int)U, th, tabs, L, (int)n_l, b, (int)H, S_B, nullptr);
    FCD_LAUNCH_CHECK();
    if (slots) {
        hipLaunchKernelGGL(nan_fold_kernel, dim3(1), dim3(FCD_NAN_SLOTS), 0, s, slots, nan_counts);
        FCD_LAUNCH_CHECK();
    }
    return FCD_OK;
}
