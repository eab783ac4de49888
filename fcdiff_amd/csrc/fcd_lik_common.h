// The arithmetic of K_lik (fcd_lik.hip) as inline helpers, for K_lik_shared (fcd_lik_shared.hip) and the patient-or-control
// kernel (fcd_member.hip): the parameters as the kernels read them, the per-item ln M_kl, the ln N_k of S_B and the S_B
// blocks, statement for statement as lik_kernel has them.
// lik_kernel keeps its own text: routed through these helpers its MISSING form compiles to other instructions (same
// results, a different schedule), and the table kernel of the unshared fit is not changed by the shared one.  What
// binds the two copies is a test: S_B of both launches is compared bit for bit, and L against the patient sum of lM.
#pragma once
#include "fcd_common.h"
#include "fcd_fastmath.h"

namespace {

struct LikTheta {
    double mu[3];
    double sigma[3];
    double inv_sigma[3];   // 1 / sigma_k
    double pdf_scale[3];   // 1 / sqrt(2 pi) / sigma_k  (the reference's two divisions applied to 1.0)
    double lnsigma[3];
    double eps[3];       // _eval_M_eps(eta, epsilon, l), l = 0,1,2
    double omeps_half[3];  // (1 - eps_l) * 0.5, the reference's evaluation order
    double cmin;           // min over l of min(eps_l, omeps_half_l): every M_kl >= cmin * (N_0 + N_1 + N_2)
};

constexpr double kSqrt2Pi = 2.5066282746310002;      // numpy: sqrt(2*pi)
constexpr double kLogSqrt2Pi = 0.9189385332046727;   // numpy: log(sqrt(2*pi))

constexpr int LIK_BLOCK = 256;

struct LikTabs {
    double exp_tab[FCD_EXP_CELLS];
    fcd_log_cell log_tab[FCD_LOG_CELLS];
};

// theta12 (host) -> LikTheta, _eval_M_eps of fit.py:433-444 in the same operation order
static inline void lik_theta_make(const double *theta, LikTheta &th) {
    const double eta = theta[1], epsilon = theta[2];
    for (int k = 0; k < 3; ++k) {
        th.mu[k] = theta[6 + k];
        th.sigma[k] = theta[9 + k];
        th.inv_sigma[k] = 1.0 / theta[9 + k];
        th.pdf_scale[k] = 1.0 / kSqrt2Pi / theta[9 + k];
        th.lnsigma[k] = log(theta[9 + k]);
    }
    th.eps[0] = 1 - epsilon;
    th.eps[1] = epsilon;
    double e2 = eta * epsilon;
    e2 += (1 - eta) * (1 - epsilon);
    th.eps[2] = e2;
    for (int l = 0; l < 3; ++l) th.omeps_half[l] = (1 - th.eps[l]) * 0.5;
    th.cmin = th.eps[0];
    for (int l = 0; l < 3; ++l) {
        if (!(th.eps[l] >= th.cmin)) th.cmin = th.eps[l];
        if (!(th.omeps_half[l] >= th.cmin)) th.cmin = th.omeps_half[l];
    }
    if (!(th.cmin > 0.0)) th.cmin = 0.0;          // eps outside (0, 1): no floor, every item takes the general log
}

// The three Normal densities of one bt item (fit.py:115).  The kernel is ALU-bound and an fp64 division is ~15
// instructions, so the three divisions per component are multiplications by host-side reciprocals (<= 2 ulp of the
// density, ~1e-16 relative in log M) ... except at the edge of the double range, where the reference's own roundings
// decide whether the density is 0 (lM = -inf) or a subnormal: there its operations are redone exactly (rare branch).
__device__ __forceinline__ void lik_densities(double x, const LikTheta &th, const double *etab, double N[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double d = x - th.mu[k];
        const double z = d * th.inv_sigma[k];
        N[k] = fcd_exp_neg((z * z) / 2.0, etab) * th.pdf_scale[k];
        if (N[k] < 1e-290) {
            const double ze = d / th.sigma[k];
            N[k] = exp(-(ze * ze) / 2.0) / kSqrt2Pi / th.sigma[k];
        }
    }
}

// v[k*3+l] = ln M_kl from the densities (fit.py:122, :430); js = the two other components in ascending order
// (fit.py:428-429).  All nine M_kl are >= cmin * (N_0 + N_1 + N_2): one comparison shows them positive, finite and
// normal and sends them through the branch-free log; the rare item at the edge of the double range (or eps in {0, 1})
// takes the general log, -inf for an underflowed density like np.log.
__device__ __forceinline__ void lik_logs(const double N[3], const LikTheta &th, const fcd_log_cell *ltab, double v[9]) {
    const double others[3] = {N[1] + N[2], N[0] + N[2], N[0] + N[1]};
    const double floor_M = th.cmin * (N[0] + others[0]);
    if (floor_M >= 4.5e-308 && floor_M < __builtin_inf()) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int l = 0; l < 3; ++l) v[k * 3 + l] = fcd_log_normal(th.eps[l] * N[k] + th.omeps_half[l] * others[k], ltab);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int l = 0; l < 3; ++l) v[k * 3 + l] = log(th.eps[l] * N[k] + th.omeps_half[l] * others[k]);
    }
}

// ln N(x; mu_k, sigma_k) = -z*z/2 - log(sqrt(2 pi)) - log(sigma_k), k = 0,1,2 (fit.py:114): the terms of S_B, and the control
// side of fcd_member_loglik
__device__ __forceinline__ void lik_normal_logs(double x, const LikTheta &th, double &l0, double &l1, double &l2) {
    const double z0 = (x - th.mu[0]) / th.sigma[0];
    const double z1 = (x - th.mu[1]) / th.sigma[1];
    const double z2 = (x - th.mu[2]) / th.sigma[2];
    l0 = -(z0 * z0) / 2.0 - kLogSqrt2Pi - th.lnsigma[0];
    l1 = -(z1 * z1) / 2.0 - kLogSqrt2Pi - th.lnsigma[1];
    l2 = -(z2 * z2) / 2.0 - kLogSqrt2Pi - th.lnsigma[2];
}

// An S_B block: 16 lanes per edge, S_B[c,k] = sum_h ( -z*z/2 - log(sqrt(2 pi)) - log(sigma_k) )  (fit.py:114, :171);
// `sb_block` is the block's index among the S_B blocks.  MISSING: a NaN b adds 0 (and lpB holds 0); the block's NaN
// count goes to slot line (blockIdx.x % FCD_NAN_SLOTS), word 0, through `blk_nan` (the kernel's __shared__ int).
template <bool MISSING>
__device__ __forceinline__ void lik_sb_block(unsigned sb_block, int tid, const double *__restrict__ b, int64_t C, int H,
                                             const LikTheta &th, double *__restrict__ S_B, double *__restrict__ lpB,
                                             unsigned long long *__restrict__ nan_slots, int *blk_nan) {
    const int sub = tid & 15;
    const int64_t c = (int64_t)sb_block * 16 + (tid >> 4);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int nan_b = 0;
    if (MISSING && tid == 0) *blk_nan = 0;
    if (c < C) {
        const double *row = b + c * H;
        for (int h = sub; h < H; h += 16) {
            const double x = row[h];
            double l0, l1, l2;
            lik_normal_logs(x, th, l0, l1, l2);
            if (MISSING) {
                const bool miss = __builtin_isnan(x);        // unobserved: ln N integrates to ln 1 = 0
                l0 = miss ? 0.0 : l0;
                l1 = miss ? 0.0 : l1;
                l2 = miss ? 0.0 : l2;
                nan_b += miss;
            }
            if (lpB) {
                double *o = lpB + (c * H + h) * 3;
                o[0] = l0; o[1] = l1; o[2] = l2;
            }
            s0 += l0; s1 += l1; s2 += l2;
        }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o, 16);
        s1 += __shfl_xor(s1, o, 16);
        s2 += __shfl_xor(s2, o, 16);
    }
    if (c < C && sub == 0) {
        S_B[c * 3 + 0] = s0;
        S_B[c * 3 + 1] = s1;
        S_B[c * 3 + 2] = s2;
    }
    if (MISSING) {
        __syncthreads();
        if (nan_b) atomicAdd(blk_nan, nan_b);
        __syncthreads();
        if (tid == 0 && *blk_nan && nan_slots)
            atomicAdd(&nan_slots[(blockIdx.x % FCD_NAN_SLOTS) * 16 + 0], (unsigned long long)*blk_nan);
    }
}

// n_missing2 = the sums of the slot lines, which are left zero again (one block of FCD_NAN_SLOTS threads)
__global__ __launch_bounds__(FCD_NAN_SLOTS) void nan_fold_kernel(unsigned long long *__restrict__ nan_slots,
                                                                 int64_t *__restrict__ n_missing2) {
    __shared__ unsigned long long part[FCD_NAN_SLOTS / 64][2];
    unsigned long long *line = nan_slots + threadIdx.x * 16;
    unsigned long long v[2] = {line[0], line[1]};
    line[0] = 0;
    line[1] = 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o);
        if (lane == 0) part[wave][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long t = 0;
        for (int q = 0; q < FCD_NAN_SLOTS / 64; ++q) t += part[q][threadIdx.x];
        n_missing2[threadIdx.x] = (int64_t)t;
    }
}

}  // namespace
