// Scoring new patients against a fitted model: per-patient likelihood measures.
//
// Given the template F and theta, patients are independent in the IAR model (doc/methods.rst, the generative model), so a
// new patient's anomaly map and its predictive likelihood need no refit.  The q_R update, the table kernel, the r pass and
// the tallies are reused as they are; what is new here is the per-patient likelihood measure of each fitter:
//   patient_elbo_edges / patient_elbo_fold   variational fit: the per-patient split of the energy terms that involve
//                             patients, E_lM[u], E_lp_R[u], E_lq_R[u], and elbo[u] = E_lM + E_lp_R - E_lq_R, a lower bound
//                             on E_{q_F} log p(bt_u | F).  lM is read once, edge slices per workgroup, lanes over patients;
//                             the slices are folded in slice order by one wave per patient (bitwise repeatable, and a
//                             patient's result does not depend on the other patients in the call).
//   score_ais_kernel / score_ais_fold        sampler: one step of annealed importance sampling over r with each chain's
//                             template f_g held.  l_gu = sum_c lM[c, u, f_gc, l(r_gnu, r_gmu)] (true endpoints of c, the mixture
//                             case of gibbs_logjoint_kernel) at the current r, w[g, u] += (beta - beta_prev) l_gu, and
//                             beta * lM into the working table the r pass reads next (the r pass itself is not touched:
//                             tempering is carried entirely by its table).
//   score_ais_finish          per patient {max_g w, sum_g exp(w - max), sum_g exp(2 (w - max)), G}: what the host pools over
//                             ranks into log_pred, its standard error and the effective sample size.
#include "fcd_common.h"

namespace {

__device__ inline double xlogy0(double q, double lq) { return q == 0.0 ? 0.0 : q * lq; }

__device__ inline double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- per-patient ELBO ----------------------------------------------------------------------
constexpr int EL_WAVES = 4;
constexpr int EL_MIN_EDGES = 64;      // edges per slice at least
constexpr int EL_MAX_SLICES = 1024;

// the number of edge slices depends on C alone: a patient's sums are the same whatever U is
static inline int64_t elbo_slices(int64_t C) {
    int64_t s = (C + EL_MIN_EDGES - 1) / EL_MIN_EDGES;
    return s > EL_MAX_SLICES ? EL_MAX_SLICES : s;
}

// grid (slices, ceil(U / 64)), EL_WAVES waves: wave v takes edges c0 + v, c0 + v + EL_WAVES, ... of the slice, lane = patient.
// part[s * U + u] = sum over the slice's edges of sum_k q_F[c,k] sum_l w_l(c,u) lM[c,u,k,l]   (fit.py:489-511 per patient)
__global__ __launch_bounds__(64 * EL_WAVES) void patient_elbo_edges(const double *__restrict__ lq_F, const double *__restrict__ lq_R,
                                                                    const double *__restrict__ lM, int64_t C, int U, int S,
                                                                    double *__restrict__ part) {
    __shared__ double red[EL_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x;
    const int u = blockIdx.y * 64 + lane;
    const int64_t c0 = C * s / S, c1 = C * (s + 1) / S;
    double e = 0.0;
    if (u < U) {
        for (int64_t c = c0 + wave; c < c1; c += EL_WAVES) {
            int n, m;
            fcd_edge_to_pair(c, n, m);
            const double q0n = exp(lq_R[((int64_t)n * U + u) * 2 + 0]);
            const double q1n = exp(lq_R[((int64_t)n * U + u) * 2 + 1]);
            const double q0m = exp(lq_R[((int64_t)m * U + u) * 2 + 0]);
            const double q1m = exp(lq_R[((int64_t)m * U + u) * 2 + 1]);
            const double w0 = q0n * q0m;
            const double w1 = q1n * q1m;
            double w2 = q0n * q1m;
            w2 += q1n * q0m;
            const double *p = lM + (c * U + u) * 9;
            const double t0 = (w0 * p[0] + w1 * p[1]) + w2 * p[2];
            const double t1 = (w0 * p[3] + w1 * p[4]) + w2 * p[5];
            const double t2 = (w0 * p[6] + w1 * p[7]) + w2 * p[8];
            e += (exp(lq_F[c * 3 + 0]) * t0 + exp(lq_F[c * 3 + 1]) * t1) + exp(lq_F[c * 3 + 2]) * t2;
        }
    }
    red[wave][lane] = e;
    __syncthreads();
    if (wave == 0 && u < U) {
        double v = red[0][lane];
#pragma unroll
        for (int j = 1; j < EL_WAVES; ++j) v += red[j][lane];
        part[(int64_t)s * U + u] = v;
    }
}

// one wave per patient: the slices in lane order (lane j: s = j, j + 64, ...) and the region terms (lane j: n = j, j + 64, ...),
// each folded by the wave sum.  out4[u] = {E_lM, E_lp_R, E_lq_R, elbo}.
__global__ __launch_bounds__(256) void patient_elbo_fold(const double *__restrict__ part, const double *__restrict__ lq_R,
                                                         const double *__restrict__ hyper, int Nreg, int U, int S,
                                                         double *__restrict__ out4) {
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= U) return;
    double eM = 0.0, eR = 0.0, eq = 0.0;
    for (int s = lane; s < S; s += 64) eM += part[(int64_t)s * U + u];
    const double lnpi0 = hyper[FCD_H_LNPI0], lnpi1 = hyper[FCD_H_LNPI1];
    for (int n = lane; n < Nreg; n += 64) {
        const double l0 = lq_R[((int64_t)n * U + u) * 2 + 0], l1 = lq_R[((int64_t)n * U + u) * 2 + 1];
        const double q0 = exp(l0), q1 = exp(l1);
        eR += q0 * lnpi0 + q1 * lnpi1;                   // fit.py:486
        eq += xlogy0(q0, l0) + xlogy0(q1, l1);           // fit.py:539
    }
    eM = fcd_wave_sum(eM);
    eR = fcd_wave_sum(eR);
    eq = fcd_wave_sum(eq);
    if (lane == 0) {
        out4[(int64_t)u * 4 + 0] = eM;
        out4[(int64_t)u * 4 + 1] = eR;
        out4[(int64_t)u * 4 + 2] = eq;
        out4[(int64_t)u * 4 + 3] = (eM + eR) - eq;
    }
}

// ---- annealed importance sampling ------------------------------------------------------------
constexpr int AIS_TE = 256;           // edges per LDS tile: their f bytes (16 KiB)
constexpr int AIS_MAX_WAVES = 16;
constexpr int AIS_MIN_EDGES = 64;
constexpr size_t AIS_PART_MAX = (size_t)256 << 20;

// grid (GW, S slices, patient groups), NW waves: workgroup (w, s, pg) takes chain word w, the edges of slice s and the
// patients u = pg * NW * PT + j * NW + wave (j < PT), one lane per chain.  The f bytes of each edge tile are staged in LDS
// once and shared by every wave (f_state is read once per chain word for up to NW * PT = 128 patients); r comes as
// wave-uniform bit-plane words; the table value is one gather per (edge, patient, chain).  The loop over a slice's edges is
// a chain of memory round trips per edge (r words, then the gather): the slices are made small enough for 8 waves per CU.
// part[(s * U + u) * GP + g] = sum over the slice's edges of lM[c, u, f_gc, l(r_gnu, r_gmu)].
template <int PT>
__global__ __launch_bounds__(64 * AIS_MAX_WAVES) void score_ais_kernel(const double *__restrict__ lM, const uint8_t *__restrict__ f_state,
                                                                       const uint64_t *__restrict__ r_bits, int Nreg, int U, int64_t C,
                                                                       int S, double *__restrict__ part) {
    __shared__ uint8_t fT[AIS_TE * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, NW = blockDim.x >> 6;
    const int w = blockIdx.x, s = blockIdx.y;
    const int GW = gridDim.x;
    const int u0 = blockIdx.z * NW * PT + wave;
    const int64_t c0 = C * s / S, c1 = C * (s + 1) / S;
    const uint64_t *rw = r_bits + (int64_t)w * Nreg * U;
    // the endpoints (n, m) of edge c walk the lower triangle in order, kept wave-uniform (scalar registers): the r words are
    // scalar loads that depend on nothing of the previous edge, so the loads of consecutive edges overlap
    int n, m;
    fcd_edge_to_pair(c0, n, m);
    double acc[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) acc[j] = 0.0;
    for (int64_t ct = c0; ct < c1; ct += AIS_TE) {
        const int ne = (int)(c1 - ct < AIS_TE ? c1 - ct : AIS_TE);
        __syncthreads();                                   // the previous tile is read
        const uint32_t *src = reinterpret_cast<const uint32_t *>(f_state + ((int64_t)w * C + ct) * 64);
        uint32_t *dst = reinterpret_cast<uint32_t *>(fT);
        for (int i = threadIdx.x; i < ne * 16; i += blockDim.x) dst[i] = src[i];
        __syncthreads();
#pragma unroll 2
        for (int i = 0; i < ne; ++i) {
            const int k = min((int)fT[i * 64 + lane], 2);     // (f is in {0, 1, 2}; the clamp keeps a stray byte in bounds)
            const double *rec = lM + (ct + i) * U * 9 + k * 3;
            const uint64_t *rn = rw + (int64_t)n * U, *rm = rw + (int64_t)m * U;
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                const int u = u0 + j * NW;
                if (u < U) {
                    const uint32_t a = (uint32_t)((rn[u] >> lane) & 1ull);
                    const uint32_t b = (uint32_t)((rm[u] >> lane) & 1ull);
                    const int l = (a & b) ? 1 : ((a ^ b) ? 2 : 0);
                    acc[j] += rec[(int64_t)u * 9 + l];
                }
            }
            if (++m == n) {
                ++n;
                m = 0;
            }
        }
    }
    const int64_t GP = (int64_t)GW * 64;
#pragma unroll
    for (int j = 0; j < PT; ++j) {
        const int u = u0 + j * NW;
        if (u < U) part[((int64_t)s * U + u) * GP + (int64_t)w * 64 + lane] = acc[j];
    }
}

// w[g, u] += (beta - beta_prev) * sum_s part[s, u, g] (slices in order), then lM_beta = beta * lM (when asked).
__global__ __launch_bounds__(256) void score_ais_fold(const double *__restrict__ part, int S, int U, int64_t G, int64_t GP,
                                                      double dbeta, double *__restrict__ w, const double *__restrict__ lM,
                                                      double beta, double *__restrict__ lM_beta, int64_t n_tab) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n_w = (int64_t)U * G;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_w; i += stride) {
        const int64_t u = i / G, g = i % G;
        double l = 0.0;
        for (int s = 0; s < S; ++s) l += part[((int64_t)s * U + u) * GP + g];
        w[g * U + u] += dbeta * l;
    }
    if (lM_beta) {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_tab; i += stride) lM_beta[i] = beta * lM[i];
    }
}

// one wave per patient: {max_g w, sum exp(w - max), sum exp(2 (w - max)), G}; chains in lane order, folded by the wave.
// max = -inf (every weight zero) leaves both sums 0.
__global__ __launch_bounds__(256) void score_ais_finish(const double *__restrict__ w, int U, int64_t G, double *__restrict__ out4) {
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= U) return;
    double mx = -INFINITY;
    for (int64_t g = lane; g < G; g += 64) mx = fmax(mx, w[g * U + u]);
    mx = wave_max(mx);
    double s1 = 0.0, s2 = 0.0;
    if (mx > -INFINITY) {
        for (int64_t g = lane; g < G; g += 64) {
            const double e = exp(w[g * U + u] - mx);
            s1 += e;
            s2 += e * e;
        }
    }
    s1 = fcd_wave_sum(s1);
    s2 = fcd_wave_sum(s2);
    if (lane == 0) {
        out4[(int64_t)u * 4 + 0] = mx;
        out4[(int64_t)u * 4 + 1] = s1;
        out4[(int64_t)u * 4 + 2] = s2;
        out4[(int64_t)u * 4 + 3] = (double)G;
    }
}

int score_shape(fcd_ctx *ctx, int64_t Nreg, int64_t U) {
    if (Nreg < 2 || U < 1) return fcd_fail(ctx, FCD_ERR_SHAPE, "need Nreg >= 2 and U >= 1 (Nreg=%lld, U=%lld)", Nreg, U);
    if (Nreg > 46340 || U > (1 << 24)) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "Nreg=%lld / U=%lld too large", Nreg, U);
    return FCD_OK;
}

}  // namespace

extern "C" int fcd_vb_patient_elbo(fcd_ctx *ctx, const double *lq_F, const double *lq_R, const double *lM, const double *hyper,
                                   int64_t Nreg, int64_t U, double *out4, fcd_stream stream) {
    if (!ctx || !lq_F || !lq_R || !lM || !hyper || !out4) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_vb_patient_elbo: null pointer");
    int rc = score_shape(ctx, Nreg, U);
    if (rc) return rc;
    if ((U + 63) / 64 > 65535) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_vb_patient_elbo: U=%lld exceeds the grid", U);
    const int64_t C = fcd_tri(Nreg);
    const int64_t S = elbo_slices(C);
    rc = fcd_ws_reserve(ctx, (size_t)S * (size_t)U * sizeof(double));
    if (rc) return rc;
    double *part = (double *)ctx->ws.p;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(patient_elbo_edges, dim3((unsigned)S, (unsigned)((U + 63) / 64)), dim3(64 * EL_WAVES), 0, s, lq_F, lq_R, lM,
                       C, (int)U, (int)S, part);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(patient_elbo_fold, dim3((unsigned)((U + 3) / 4)), dim3(256), 0, s, (const double *)part, lq_R, hyper,
                       (int)Nreg, (int)U, (int)S, out4);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_score_ais_step(fcd_ctx *ctx, const double *lM, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg,
                                  int64_t U, int64_t G, double beta_prev, double beta, double *w, double *lM_beta,
                                  fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!lM || !f_state || !r_bits || !w) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_score_ais_step: null pointer");
    FCD_ALIGN16(ctx, "fcd_score_ais_step", "f_state", f_state);          // score_ais_kernel stages its lines as 32-bit words
    if (lM_beta == w || (const double *)lM_beta == lM)
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_score_ais_step: lM_beta must not alias lM or w");
    const int NW = (int)(U < AIS_MAX_WAVES ? U : AIS_MAX_WAVES);
    const int64_t per_wave = (U + NW - 1) / NW;
    const int PT = per_wave <= 1 ? 1 : per_wave <= 2 ? 2 : per_wave <= 4 ? 4 : 8;
    const int64_t NPG = (U + (int64_t)NW * PT - 1) / ((int64_t)NW * PT);
    if (NPG > 65535) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_score_ais_step: U=%lld exceeds the grid", U);
    const int64_t GP = (int64_t)g.GW * 64;
    // edge slices: enough for two workgroups and 8 waves per CU (a development measurement at cfg3, not recorded in
    // profiles/: fewer, longer slices of the same waves were slower), at least AIS_MIN_EDGES edges per slice, partials
    // within AIS_PART_MAX
    const int64_t wgs = (int64_t)g.GW * NPG, wg_waves = wgs * NW;
    int64_t S = (2 * (int64_t)ctx->num_cu + wgs - 1) / wgs;
    const int64_t S_waves = (8 * (int64_t)ctx->num_cu + wg_waves - 1) / wg_waves;
    if (S < S_waves) S = S_waves;
    const int64_t s_edges = (g.C + AIS_MIN_EDGES - 1) / AIS_MIN_EDGES;
    if (S > s_edges) S = s_edges;
    const int64_t s_bytes = (int64_t)(AIS_PART_MAX / ((size_t)U * (size_t)GP * sizeof(double)));
    if (S > s_bytes) S = s_bytes;
    if (S > 65535) S = 65535;
    if (S < 1) S = 1;
    rc = fcd_ws_reserve(ctx, (size_t)S * (size_t)U * (size_t)GP * sizeof(double));
    if (rc) return rc;
    double *part = (double *)ctx->ws.p;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)g.GW, (unsigned)S, (unsigned)NPG), block((unsigned)(64 * NW));
    if (PT == 1)
        hipLaunchKernelGGL(score_ais_kernel<1>, grid, block, 0, s, lM, f_state, r_bits, (int)Nreg, (int)U, g.C, (int)S, part);
    else if (PT == 2)
        hipLaunchKernelGGL(score_ais_kernel<2>, grid, block, 0, s, lM, f_state, r_bits, (int)Nreg, (int)U, g.C, (int)S, part);
    else if (PT == 4)
        hipLaunchKernelGGL(score_ais_kernel<4>, grid, block, 0, s, lM, f_state, r_bits, (int)Nreg, (int)U, g.C, (int)S, part);
    else
        hipLaunchKernelGGL(score_ais_kernel<8>, grid, block, 0, s, lM, f_state, r_bits, (int)Nreg, (int)U, g.C, (int)S, part);
    FCD_LAUNCH_CHECK();
    const int64_t n_tab = g.C * U * 9;
    const int64_t work = (U * G > n_tab ? U * G : n_tab);
    int64_t blocks = (work + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cu * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(score_ais_fold, dim3((unsigned)blocks), dim3(256), 0, s, (const double *)part, (int)S, (int)U, G, GP,
                       beta - beta_prev, w, lM, beta, lM_beta, n_tab);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_score_ais_finish(fcd_ctx *ctx, const double *w, int64_t U, int64_t G, double *out4, fcd_stream stream) {
    if (!ctx || !w || !out4) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_score_ais_finish: null pointer");
    if (U < 1 || G < 1) return fcd_fail(ctx, FCD_ERR_SHAPE, "fcd_score_ais_finish: U=%lld G=%lld", U, G);
    if ((U + 3) / 4 > (1ll << 31) - 1) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_score_ais_finish: U=%lld", U);
    hipLaunchKernelGGL(score_ais_finish, dim3((unsigned)((U + 3) / 4)), dim3(256), 0, (hipStream_t)stream, w, (int)U, G, out4);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
