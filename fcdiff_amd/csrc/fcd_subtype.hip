// The subtype-region model (latent patient subtypes, fitted by mean-field VB): the two passes over the per-patient table
// lM (C, U, 3, 3) that every outer iteration makes.  With responsibilities s[u, g] = q(z_u = g) the expected collapsed
// log-likelihood is the unshared model's E_lM term at G pseudo-patients whose table is the weighted sum L below, so the
// q_F / q_R updates, the theta step and the energy run unchanged at patient extent G on L; what is new is
//   weighted_tables_kernel    L[c, g, k, l] = sum_u s[u, g] lM[c, u, k, l].  One wave per edge: its row lM[c] is 9 U contiguous
//                             doubles, read 63 at a time -- lane j takes entry j % 9 of patient j / 9 + 7 i -- so every load
//                             is one contiguous 504-byte run.  A lane keeps G sums over its patients in ascending order; the
//                             seven lanes of an entry are folded in lane order through LDS.  No atomics: two calls agree
//                             bit for bit.  A weight that is exactly 0 adds 0.0 whatever the entry (-inf included).
//   subtype_loglik_edges / subtype_loglik_fold
//                             E[u, g] = sum_c sum_k q_F[c,k] sum_l w_l^g(c) lM[c,u,k,l], w^g the mixture-case weights of
//                             subtype g's q_R at the true endpoints of c: patient_elbo_edges' mapping (fcd_score.hip: edge
//                             slices per workgroup, lanes over patients, the slices folded in slice order by one wave per
//                             patient) with G sums per lane, so lM is read once for all G.  q_F = exp(lq_F) and
//                             q_R = exp(lq_R) are made once per call by subtype_exp_kernel (patient_elbo_edges takes the
//                             seven exponentials per edge and lane); the weights are wave-uniform reads of that block.
//                             The number of slices depends on C alone and a lane reads nothing of another patient: E[u, :]
//                             does not depend on the other patients of the call.
// Both are templates over G = 1 .. SUBTYPE_MAX so that the G sums of a lane are registers.
#include "fcd_common.h"

namespace {

constexpr int SUBTYPE_MAX = 8;

// ---- weighted table sum ------------------------------------------------------------------------
constexpr int WT_WAVES = 4;           // edges per workgroup, one per wave
constexpr int WT_PAT = 7;             // patients per wave and load: 7 * 9 = 63 lanes

template <int G>
__global__ __launch_bounds__(64 * WT_WAVES) void weighted_tables_kernel(const double *__restrict__ lM, const double *__restrict__ resp,
                                                                        int64_t C, int U, double *__restrict__ L) {
    __shared__ double red[WT_WAVES][G][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t c = (int64_t)blockIdx.x * WT_WAVES + wave;
    const int du = lane / 9, kl = lane - du * 9;
    double acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = 0.0;
    if (c < C && lane < 9 * WT_PAT) {
        const double *row = lM + c * U * 9;
        for (int u = du; u < U; u += WT_PAT) {
            const double v = row[(int64_t)u * 9 + kl];
            const double *su = resp + (int64_t)u * G;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const double s = su[g];
                acc[g] += s == 0.0 ? 0.0 : s * v;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) red[wave][g][lane] = acc[g];
    __syncthreads();
    if (c < C) {
        for (int i = lane; i < 9 * G; i += 64) {
            const int g = i / 9, k = i - g * 9;
            double v = red[wave][g][k];
#pragma unroll
            for (int j = 1; j < WT_PAT; ++j) v += red[wave][g][k + 9 * j];
            L[(c * G + g) * 9 + k] = v;
        }
    }
}

// ---- per-(patient, subtype) expected log-likelihood ----------------------------------------------
constexpr int SL_WAVES = 4;
constexpr int SL_MIN_EDGES = 64;      // edges per slice at least
constexpr int SL_MAX_SLICES = 1024;

// the number of edge slices depends on C alone: a patient's sums are the same whatever U is
static inline int64_t loglik_slices(int64_t C) {
    int64_t s = (C + SL_MIN_EDGES - 1) / SL_MIN_EDGES;
    return s > SL_MAX_SLICES ? SL_MAX_SLICES : s;
}

// qF (C, 3) = exp(lq_F), qR (Nreg, G, 2) = exp(lq_R): grid-stride over both
__global__ __launch_bounds__(256) void subtype_exp_kernel(const double *__restrict__ lq_F, const double *__restrict__ lq_R, int64_t nF,
                                                          int64_t nR, double *__restrict__ qF, double *__restrict__ qR) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nF + nR; i += stride) {
        if (i < nF)
            qF[i] = exp(lq_F[i]);
        else
            qR[i - nF] = exp(lq_R[i - nF]);
    }
}

// grid (slices, ceil(U / 64)), SL_WAVES waves: wave v takes edges c0 + v, c0 + v + SL_WAVES, ... of the slice, lane = patient.
// part[(s * U + u) * G + g] = sum over the slice's edges of sum_k q_F[c,k] sum_l w_l^g(c) lM[c,u,k,l], the products and sums
// of an edge taken as patient_elbo_edges takes them.
template <int G>
__global__ __launch_bounds__(64 * SL_WAVES) void subtype_loglik_edges(const double *__restrict__ qF, const double *__restrict__ qR,
                                                                      const double *__restrict__ lM, int64_t C, int U, int S,
                                                                      double *__restrict__ part) {
    __shared__ double red[SL_WAVES][G][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = blockIdx.x;
    const int u = blockIdx.y * 64 + lane;
    const int64_t c0 = C * s / S, c1 = C * (s + 1) / S;
    double e[G];
#pragma unroll
    for (int g = 0; g < G; ++g) e[g] = 0.0;
    if (u < U && c0 + wave < c1) {
        // the endpoints (n, m) of edge c walk the lower triangle SL_WAVES edges at a time, wave-uniform
        int n, m;
        fcd_edge_to_pair(c0 + wave, n, m);
        for (int64_t c = c0 + wave; c < c1; c += SL_WAVES) {
            const double *p = lM + (c * U + u) * 9;
            const double p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4], p5 = p[5], p6 = p[6], p7 = p[7], p8 = p[8];
            const double f0 = qF[c * 3 + 0], f1 = qF[c * 3 + 1], f2 = qF[c * 3 + 2];
            const double *rn = qR + (int64_t)n * G * 2, *rm = qR + (int64_t)m * G * 2;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const double q0n = rn[g * 2 + 0], q1n = rn[g * 2 + 1];
                const double q0m = rm[g * 2 + 0], q1m = rm[g * 2 + 1];
                const double w0 = q0n * q0m;
                const double w1 = q1n * q1m;
                double w2 = q0n * q1m;
                w2 += q1n * q0m;
                const double t0 = (w0 * p0 + w1 * p1) + w2 * p2;
                const double t1 = (w0 * p3 + w1 * p4) + w2 * p5;
                const double t2 = (w0 * p6 + w1 * p7) + w2 * p8;
                e[g] += (f0 * t0 + f1 * t1) + f2 * t2;
            }
            m += SL_WAVES;
            while (m >= n) {
                m -= n;
                ++n;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) red[wave][g][lane] = e[g];
    __syncthreads();
    if (wave == 0 && u < U) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            double v = red[0][g][lane];
#pragma unroll
            for (int j = 1; j < SL_WAVES; ++j) v += red[j][g][lane];
            part[((int64_t)s * U + u) * G + g] = v;
        }
    }
}

// one wave per patient: for every subtype the slices in lane order (lane j: s = j, j + 64, ...), folded by the wave sum
__global__ __launch_bounds__(256) void subtype_loglik_fold(const double *__restrict__ part, int U, int G, int S, double *__restrict__ E) {
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= U) return;
    for (int g = 0; g < G; ++g) {
        double v = 0.0;
        for (int s = lane; s < S; s += 64) v += part[((int64_t)s * U + u) * G + g];
        v = fcd_wave_sum(v);
        if (lane == 0) E[(int64_t)u * G + g] = v;
    }
}

template <int G>
void weighted_tables_launch(const double *lM, const double *resp, int64_t C, int64_t U, double *L, hipStream_t s) {
    hipLaunchKernelGGL(weighted_tables_kernel<G>, dim3((unsigned)((C + WT_WAVES - 1) / WT_WAVES)), dim3(64 * WT_WAVES), 0, s, lM, resp,
                       C, (int)U, L);
}

template <int G>
void loglik_edges_launch(const double *qF, const double *qR, const double *lM, int64_t C, int64_t U, int64_t S, double *part,
                         hipStream_t s) {
    hipLaunchKernelGGL(subtype_loglik_edges<G>, dim3((unsigned)S, (unsigned)((U + 63) / 64)), dim3(64 * SL_WAVES), 0, s, qF, qR, lM, C,
                       (int)U, (int)S, part);
}

// FCD_SUBTYPE_DISPATCH(fn, G, args...): fn<G>(args...) for the run-time G in 1 .. SUBTYPE_MAX
#define FCD_SUBTYPE_DISPATCH(fn, G, ...) \
    switch (G) {                         \
        case 1: fn<1>(__VA_ARGS__); break; \
        case 2: fn<2>(__VA_ARGS__); break; \
        case 3: fn<3>(__VA_ARGS__); break; \
        case 4: fn<4>(__VA_ARGS__); break; \
        case 5: fn<5>(__VA_ARGS__); break; \
        case 6: fn<6>(__VA_ARGS__); break; \
        case 7: fn<7>(__VA_ARGS__); break; \
        default: fn<8>(__VA_ARGS__); break; \
    }

}  // namespace

extern "C" int fcd_lik_weighted_tables(fcd_ctx *ctx, const double *lM, const double *resp, int64_t C, int64_t U, int64_t G, double *L,
                                       fcd_stream stream) {
    if (!ctx || !lM || !resp || !L) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_weighted_tables: null pointer");
    if (G < 1 || G > SUBTYPE_MAX) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_weighted_tables: G=%lld, must be 1 .. %lld", G, SUBTYPE_MAX);
    if (U < 1) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_weighted_tables: U=%lld, must be >= 1", U);
    if ((const double *)L == lM) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_weighted_tables: L must not alias lM");
    if (fcd_C_to_N(C) < 0) return fcd_fail(ctx, FCD_ERR_SHAPE, "Number of connections (%lld) must be a triangular number.", C);
    if (U > (1 << 24) || (C + WT_WAVES - 1) / WT_WAVES > INT32_MAX)
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_lik_weighted_tables: C=%lld / U=%lld too large", C, U);
    hipStream_t s = (hipStream_t)stream;
    FCD_SUBTYPE_DISPATCH(weighted_tables_launch, (int)G, lM, resp, C, U, L, s)
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_vb_subtype_loglik(fcd_ctx *ctx, const double *lq_F, const double *lq_R, const double *lM, int64_t Nreg, int64_t U,
                                     int64_t G, double *E, fcd_stream stream) {
    if (!ctx || !lq_F || !lq_R || !lM || !E) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_vb_subtype_loglik: null pointer");
    if (G < 1 || G > SUBTYPE_MAX) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_vb_subtype_loglik: G=%lld, must be 1 .. %lld", G, SUBTYPE_MAX);
    if (U < 1) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_vb_subtype_loglik: U=%lld, must be >= 1", U);
    if (Nreg < 2) return fcd_fail(ctx, FCD_ERR_SHAPE, "fcd_vb_subtype_loglik: need Nreg >= 2 (Nreg=%lld)", Nreg);
    if (Nreg > 46340 || U > (1 << 24) || (U + 63) / 64 > 65535)
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_vb_subtype_loglik: Nreg=%lld / U=%lld too large", Nreg, U);
    const int64_t C = fcd_tri(Nreg);
    const int64_t S = loglik_slices(C);
    const int64_t nF = C * 3, nR = Nreg * G * 2;
    int rc = fcd_ws_reserve(ctx, (size_t)(nF + nR + S * U * G) * sizeof(double));
    if (rc) return rc;
    double *qF = (double *)ctx->ws.p, *qR = qF + nF, *part = qR + nR;
    hipStream_t s = (hipStream_t)stream;
    int64_t blocks = (nF + nR + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cu * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(subtype_exp_kernel, dim3((unsigned)blocks), dim3(256), 0, s, lq_F, lq_R, nF, nR, qF, qR);
    FCD_LAUNCH_CHECK();
    FCD_SUBTYPE_DISPATCH(loglik_edges_launch, (int)G, (const double *)qF, (const double *)qR, lM, C, U, S, part, s)
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(subtype_loglik_fold, dim3((unsigned)((U + 3) / 4)), dim3(256), 0, s, (const double *)part, (int)U, (int)G, (int)S,
                       E);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
