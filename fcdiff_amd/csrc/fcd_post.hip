// Connection-level posteriors: P(T_cu = 1), P(F~_cu = j) and P(F~_cu != F_c) given the data.
//
// Both fitters integrate T and F~ out into M_kl (doc/methods.rst:248-349, fit.py:409-444).  Conditioned on f_c = k, the
// mixture case l of (r_n, r_m) and bt_cu, the two have a closed-form law (methods.rst:70-177):
//   N_j = Normal(bt; mu_j, sigma_j),  e_l = _eval_M_eps(eta, epsilon, l),  S_k = sum_{j != k} N_j
//   M_kl              = e_l N_k + (1 - e_l)/2 S_k
//   P(T = 1 | k,l)    = pT_l (eps N_k + (1 - eps)/2 S_k) / M_kl,      pT = (0, 1, eta)
//   P(F~ = j | k,l)   = (j == k ? e_l : (1 - e_l)/2) N_j / M_kl
//   P(F~ != F | k,l)  = (1 - e_l)/2 S_k / M_kl
// A fit averages these tables over its posterior of (f_c, l_cu): the mean-field weights q_F[c,k] w_l(c,u) (variational
// fit) or the counts of (f_c = k, l_cu = l) over chains and sweeps (sampler, Rao-Blackwellised).
//
// Two kernels:
//   pair_tally_kernel   #{chains with f_c = k and mixture case l at (c,u)} of one state, added to a uint32 acc[c,u,k,l]
//                       (fcd_gibbs_pair_tally, the sweep loop's accumulator) or stored in / added to an fp64 W[c,u,k,l]
//                       (fcd_gibbs_pair_counts: the weights of the MCEM theta step).  The f bytes of an edge are read
//                       once (three ballots per chain word, kept in LDS); lanes run over patients.
//   posterior_kernel    weights + bt + theta -> the three outputs, one item per (c,u), fp64.
#include "fcd_common.h"

namespace {

constexpr int TALLY_WCH = 1024;          // chain words whose f masks one workgroup holds in LDS at a time (24 KiB)

// One workgroup per edge (grid-stride).  Step 1: every wave turns the 64 f bytes of a chain word into three masks
// (f == 0, 1, 2; inactive chains cleared) -> LDS.  Step 2: thread = patient; the r words of both endpoints give the three
// masks of the mixture cases; nine popcounts per chain word summed in registers; one read-modify-write per (c,u).
// When all the edge's masks fit (GW <= TALLY_WCH) they are made once, whatever U; otherwise once per patient block.
// acc = accumulate ? acc + counts : counts (uint32: wraps; fp64: the counts are exact integers either way).
template <typename T>
__global__ __launch_bounds__(256) void pair_tally_kernel(const uint8_t *__restrict__ f_state, const uint64_t *__restrict__ r_bits,
                                                         int Nreg, int U, int64_t C, int GW, int64_t G, int wch, bool accumulate,
                                                         T *__restrict__ acc) {
    extern __shared__ uint64_t fmask[];          // [wch][3]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int nwch = (GW + wch - 1) / wch;
    for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
        int n, m;
        fcd_edge_to_pair(c, n, m);
        for (int u0 = 0; u0 < U; u0 += blockDim.x) {
            const int u = u0 + threadIdx.x;
            uint32_t cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int wc = 0; wc < nwch; ++wc) {
                const int w0 = wc * wch;
                const int nw = min(wch, GW - w0);
                if (nwch > 1 || u0 == 0) {           // (workgroup-uniform)
                    __syncthreads();                 // the masks of the previous round are read
                    for (int j = wave; j < nw; j += nwaves) {
                        const int k = f_state[((int64_t)(w0 + j) * C + c) * 64 + lane];
                        const uint64_t act = fcd_active_mask(w0 + j, G);
                        const uint64_t b0 = __ballot(k == 0) & act, b1 = __ballot(k == 1) & act, b2 = __ballot(k == 2) & act;
                        if (lane == 0) {
                            fmask[j * 3 + 0] = b0;
                            fmask[j * 3 + 1] = b1;
                            fmask[j * 3 + 2] = b2;
                        }
                    }
                    __syncthreads();
                }
                if (u < U) {
                    for (int j = 0; j < nw; ++j) {
                        const int64_t w = w0 + j;
                        const uint64_t rn = r_bits[(w * Nreg + n) * U + u], rm = r_bits[(w * Nreg + m) * U + u];
                        const uint64_t lm[3] = {~(rn | rm), rn & rm, rn ^ rm};   // typical, both anomalous, discordant
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const uint64_t fk = fmask[j * 3 + k];
#pragma unroll
                            for (int l = 0; l < 3; ++l) cnt[k * 3 + l] += (uint32_t)__popcll(fk & lm[l]);
                        }
                    }
                }
            }
            if (u < U) {
                T *a = acc + ((int64_t)c * U + u) * 9;
#pragma unroll
                for (int j = 0; j < 9; ++j) a[j] = accumulate ? a[j] + (T)cnt[j] : (T)cnt[j];
            }
        }
    }
}

struct PostTheta {
    double mu[3], sigma[3], lsigma[3];
    double eps;           // epsilon
    double e[3];          // _eval_M_eps(eta, epsilon, l)
    double pT[3];         // p(T = 1 | l) = 0, 1, eta
};

// One item per (c,u), grid-stride.  Weights: counts (C,U,3,3) uint32 normalised per item, or -- counts == nullptr -- the
// mean-field q_F[c,k] w_l(c,u) formed from lq_F (C,1,3) and lq_R (Nreg,U,2) (the products of weights_vb_kernel).
// The densities enter only through ratios, so they are taken as exp(ln N_j - max_j ln N_j): one of them is exactly 1 and
// no item is 0/0 where all three underflow.  A (k,l) with zero weight is skipped.
// MISSING (FCD_DATA_NAN_MISSING): at a NaN bt the same closed forms with N_j = 1 for every j -- the prior law of T and F~
// given (k,l).  MISSING = false is the kernel without the flag.
template <bool MISSING>
__global__ __launch_bounds__(256) void posterior_kernel(const double *__restrict__ bt, int64_t C, int U, PostTheta th,
                                                        const uint32_t *__restrict__ counts, const double *__restrict__ lq_F,
                                                        const double *__restrict__ lq_R, double *__restrict__ p_T,
                                                        double *__restrict__ p_Ft, double *__restrict__ p_ch) {
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
        const double x = bt[i];
        double N[3];
        if (MISSING && __builtin_isnan(x)) {
            N[0] = N[1] = N[2] = 1.0;                          // unobserved: every density integrates to 1
        } else {
            double a[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double z = (x - th.mu[j]) / th.sigma[j];
                a[j] = -(z * z) / 2.0 - th.lsigma[j];            // ln N_j up to the common ln sqrt(2 pi)
            }
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
        const double inv = 1.0 / wsum;                       // (no weight at all: NaN, refused on the host for counts)
        p_T[i] = t1 * inv;
        p_ch[i] = ch * inv;
#pragma unroll
        for (int j = 0; j < 3; ++j) p_Ft[i * 3 + j] = ft[j] * inv;
    }
}

}  // namespace

template <typename T>
int fcd_pair_tally_launch(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                          const fcd_geo &g, T *acc, bool accumulate, hipStream_t s) {
    const int wch = g.GW < TALLY_WCH ? g.GW : TALLY_WCH;
    const int64_t uthreads = U < 256 ? U : 256;
    const int threads = (int)((uthreads + 63) / 64 * 64);
    int64_t blocks = g.C;
    const int64_t cap = (int64_t)ctx->num_cu * 64;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(pair_tally_kernel<T>, dim3((unsigned)blocks), dim3(threads), (size_t)wch * 3 * sizeof(uint64_t), s, f_state,
                       r_bits, (int)Nreg, (int)U, g.C, g.GW, G, wch, accumulate, acc);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
template int fcd_pair_tally_launch<uint32_t>(fcd_ctx *, const uint8_t *, const uint64_t *, int64_t, int64_t, int64_t,
                                             const fcd_geo &, uint32_t *, bool, hipStream_t);
template int fcd_pair_tally_launch<double>(fcd_ctx *, const uint8_t *, const uint64_t *, int64_t, int64_t, int64_t,
                                           const fcd_geo &, double *, bool, hipStream_t);

extern "C" int fcd_gibbs_pair_tally(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U,
                                    int64_t G, uint32_t *acc, fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!f_state || !r_bits || !acc) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_pair_tally: null pointer");
    return fcd_pair_tally_launch(ctx, f_state, r_bits, Nreg, U, G, g, acc, true, (hipStream_t)stream);
}

extern "C" int fcd_gibbs_set_pair_accumulator(fcd_ctx *ctx, uint32_t *acc, int64_t Nreg, int64_t U, int64_t every) {
    // (one buffer, given as both: "go together" cannot arise)
    return fcd_sweep_acc_set(ctx, FCD_ACC_PAIR, acc, acc, Nreg, U, every, nullptr, "fcd_gibbs_set_pair_accumulator: Nreg=%lld U=%lld",
                             nullptr, "fcd_gibbs_set_pair_accumulator: every=%lld must be >= 1");
}

extern "C" int fcd_conn_posterior_ex(fcd_ctx *ctx, const double *bt, int64_t Nreg, int64_t U, const double *theta,
                                     const uint32_t *counts, const double *lq_F, const double *lq_R, int flags, double *p_T,
                                     double *p_F_tilde, double *p_changed, fcd_stream stream) {
    if (!ctx || !bt || !theta || !p_T || !p_F_tilde || !p_changed) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_conn_posterior: null pointer");
    if (flags & ~FCD_DATA_NAN_MISSING) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_conn_posterior_ex: unknown flags 0x%x", flags);
    if ((counts != nullptr) == (lq_F != nullptr || lq_R != nullptr) || (!counts && (!lq_F || !lq_R)))
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_conn_posterior: pass counts, or lq_F and lq_R");
    if (Nreg < 2 || U < 1 || U > INT32_MAX || Nreg > 46340)
        return fcd_fail(ctx, FCD_ERR_SHAPE, "fcd_conn_posterior: Nreg=%lld U=%lld", Nreg, U);
    PostTheta th;
    const double eta = theta[1], epsilon = theta[2];
    for (int k = 0; k < 3; ++k) {
        th.mu[k] = theta[6 + k];
        th.sigma[k] = theta[9 + k];
        th.lsigma[k] = log(th.sigma[k]);
        if (!(th.sigma[k] > 0.0)) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_conn_posterior: sigma must be > 0");
    }
    th.eps = epsilon;
    th.e[0] = 1 - epsilon;                        // _eval_M_eps, fit.py:433-444
    th.e[1] = epsilon;
    double e2 = eta * epsilon;
    e2 += (1 - eta) * (1 - epsilon);
    th.e[2] = e2;
    th.pT[0] = 0.0;                               // methods.rst:81-105: both typical never, both anomalous always, else eta
    th.pT[1] = 1.0;
    th.pT[2] = eta;
    const int64_t C = fcd_tri(Nreg);
    const int64_t items = C * U;
    int64_t blocks = (items + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cu * 64;
    if (blocks > cap) blocks = cap;
    if (flags & FCD_DATA_NAN_MISSING)
        hipLaunchKernelGGL(posterior_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bt, C, (int)U, th, counts,
                           lq_F, lq_R, p_T, p_F_tilde, p_changed);
    else
        hipLaunchKernelGGL(posterior_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bt, C, (int)U, th, counts,
                           lq_F, lq_R, p_T, p_F_tilde, p_changed);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_conn_posterior(fcd_ctx *ctx, const double *bt, int64_t Nreg, int64_t U, const double *theta,
                                  const uint32_t *counts, const double *lq_F, const double *lq_R, double *p_T, double *p_F_tilde,
                                  double *p_changed, fcd_stream stream) {
    return fcd_conn_posterior_ex(ctx, bt, Nreg, U, theta, counts, lq_F, lq_R, 0, p_T, p_F_tilde, p_changed, stream);
}
