// Patient or control?  The two per-chain log-likelihoods of new subjects (UnsharedRegionFit.membership), straight from the
// correlations x (C, U'), theta and the packed chain state -- no (C, U', 3, 3) table is ever made:
//   control  lc[g, u] = sum_c ln N(x_cu; mu_k, sigma_k),            k = f_c of chain g
//   patient  lp[g, u] = sum_c ln M_{k, l}(x_cu),                    l = mixture case of (r_n, r_m) of chain g, (n, m) the true
//                                                                   endpoints of c (symmetric edge ids)
// with r one column per subject (r_cols = U') or ONE column for all of them (r_cols = 1: the shared-region model, whose
// new patient inherits the population's r).
//
//   member_kernel   a workgroup takes a slice of the edges, MB_TU subjects and 16 chain words.  Tile by tile (MB_TE edges x
//       MB_TU subjects) the 3 control logs and the 9 mixture logs of every (c, u) are made ONCE, by the arithmetic of the
//       table kernels (fcd_lik_common.h), into a 96-byte LDS record; then every wave walks the tile for a chain word of
//       its own, lanes = chains:
//         - the f byte of an edge is one coalesced 64-byte load per wave, MB_EB edges' loads issued together;
//         - the r words of (n, u) and (m, u) are wave-uniform (scalar loads); the mixture case of the 64 chains comes from
//           the two words' AND and XOR as lane masks;
//         - the two values are 8-byte LDS reads at record + k and record + 3 + 3 k + l: the lanes of a wave touch at most
//           3 + 9 different doubles of ONE record, 96 contiguous bytes = 24 banks, equal addresses broadcast: no conflict.
//       A subject outside the call (the last subject tile) has an all-zero record and a clamped r column, so the walk has
//       no branch.  A chain's sums over a slice are made by one wave in edge order.
//   member_fold     out[g, u] = the slices' sums in slice order.
// The slices depend on (C, U') and the device alone, never on G: bitwise repeatable, and chain g's numbers do not depend on
// the other chains of the call.  No atomics.
//
// FCD_DATA_NAN_MISSING: a NaN x is unobserved and adds 0 to both sides; without the flag it gives NaN, as lM would.  A
// density that underflows gives -inf, as in the tables.
#include "fcd_lik_common.h"

namespace {

constexpr int MB_NW = 16;          // waves per workgroup: a chain word each
constexpr int MB_TU = 8;           // subjects per tile: 2 x 8 fp64 accumulators per lane
constexpr int MB_TE = 64;          // edges per tile: 64 x 8 records of 96 bytes = 48 KiB (+ 8.5 KiB of log / exp tables)
constexpr int MB_REC = 12;         // doubles per record: ln N_k (3), ln M_kl (9)
constexpr int MB_EB = 8;           // edges whose f bytes are loaded together
constexpr int MB_MIN_EDGES = 16;   // edges per slice at least

// grid (S * UT, ceil(GW / MB_NW)): blockIdx.x = s * UT + subject tile.  part_c / part_p[(s * U + u) * GP + g].
template <bool BCAST, bool PATIENT>
__global__ __launch_bounds__(64 * MB_NW) void member_kernel(const double *__restrict__ x, LikTheta th, const LikTabs *__restrict__ tabs,
                                                            const uint8_t *__restrict__ f_state, const uint64_t *__restrict__ r_bits,
                                                            int Nreg, int U, int64_t C, int GW, int S, int UT, int missing,
                                                            double *__restrict__ part_c, double *__restrict__ part_p) {
    __shared__ __attribute__((aligned(16))) fcd_log_cell ltab[FCD_LOG_CELLS];
    __shared__ double etab[FCD_EXP_CELLS];
    __shared__ double tile[MB_TE * MB_TU * MB_REC];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = blockIdx.x / UT;
    const int u0 = (blockIdx.x - s * UT) * MB_TU;
    const int w = blockIdx.y * MB_NW + wave;
    const int64_t c0 = C * s / S, c1 = C * (s + 1) / S;
    for (int t = tid; t < FCD_LOG_CELLS; t += 64 * MB_NW) ltab[t] = tabs->log_tab[t];
    if (tid < FCD_EXP_CELLS) etab[tid] = tabs->exp_tab[tid];
    const int r_cols = BCAST ? 1 : U;
    const uint64_t *rw = PATIENT ? r_bits + (int64_t)(w < GW ? w : 0) * Nreg * r_cols : nullptr;
    const uint8_t *fw = f_state + (int64_t)(w < GW ? w : 0) * C * 64 + lane;
    // the r column of subject u0 + j, clamped into the call (its record is zero beyond)
    int ucol[MB_TU];
#pragma unroll
    for (int j = 0; j < MB_TU; ++j) ucol[j] = BCAST ? 0 : (u0 + j < U ? u0 + j : U - 1);
    int n, m;
    fcd_edge_to_pair(c0, n, m);
    double ac[MB_TU], ap[MB_TU];
#pragma unroll
    for (int j = 0; j < MB_TU; ++j) ac[j] = ap[j] = 0.0;
    for (int64_t ct = c0; ct < c1; ct += MB_TE) {
        const int ne = (int)(c1 - ct < MB_TE ? c1 - ct : MB_TE);
        __syncthreads();                                   // the previous tile is read (first pass: the tables are in place)
        for (int i = tid; i < ne * MB_TU; i += 64 * MB_NW) {
            const int e = i / MB_TU, j = i - e * MB_TU;
            double *rec = tile + i * MB_REC;
            const bool in = u0 + j < U;
            double xv = in ? x[(ct + e) * U + u0 + j] : th.mu[0];
            const bool zero = !in || (missing && __builtin_isnan(xv));    // unobserved: every density integrates to 1
            xv = zero ? th.mu[0] : xv;                                    // (a finite stand-in, then selects)
            double l0, l1, l2, N[3], v[9];
            lik_normal_logs(xv, th, l0, l1, l2);
            rec[0] = zero ? 0.0 : l0;
            rec[1] = zero ? 0.0 : l1;
            rec[2] = zero ? 0.0 : l2;
            if (PATIENT) {
                lik_densities(xv, th, etab, N);
                lik_logs(N, th, ltab, v);
#pragma unroll
                for (int q = 0; q < 9; ++q) rec[3 + q] = zero ? 0.0 : v[q];
            }
        }
        __syncthreads();
        if (w < GW) {
            for (int eb = 0; eb < ne; eb += MB_EB) {
                uint32_t fk[MB_EB];
#pragma unroll
                for (int e = 0; e < MB_EB; ++e) fk[e] = fw[(ct + (eb + e < ne ? eb + e : ne - 1)) * 64];
#pragma unroll
                for (int e = 0; e < MB_EB; ++e) {
                    if (eb + e >= ne) break;
                    const int kf = (int)min(fk[e], 2u);            // (f is in {0, 1, 2}; the clamp keeps a stray byte in bounds)
                    const double *rec = tile + (eb + e) * (MB_TU * MB_REC);
                    if (PATIENT) {
                        const uint64_t *rn = rw + (int64_t)n * r_cols, *rm = rw + (int64_t)m * r_cols;
                        uint32_t l[MB_TU];
                        if (BCAST) {
                            const uint64_t a = rn[0], b = rm[0];
                            const uint32_t l0 = fcd_sel_mask(fcd_sel_mask(0u, 2u, a ^ b), 1u, a & b);
#pragma unroll
                            for (int j = 0; j < MB_TU; ++j) l[j] = l0;
                        } else {
#pragma unroll
                            for (int j = 0; j < MB_TU; ++j) {
                                const uint64_t a = rn[ucol[j]], b = rm[ucol[j]];
                                l[j] = fcd_sel_mask(fcd_sel_mask(0u, 2u, a ^ b), 1u, a & b);
                            }
                        }
#pragma unroll
                        for (int j = 0; j < MB_TU; ++j) ap[j] += rec[j * MB_REC + 3 + kf * 3 + (int)l[j]];
                    }
#pragma unroll
                    for (int j = 0; j < MB_TU; ++j) ac[j] += rec[j * MB_REC + kf];
                    if (++m == n) {
                        ++n;
                        m = 0;
                    }
                }
            }
        }
    }
    if (w >= GW) return;
    const int64_t GP = (int64_t)GW * 64;
#pragma unroll
    for (int j = 0; j < MB_TU; ++j) {
        if (u0 + j < U) {
            const int64_t at = ((int64_t)s * U + u0 + j) * GP + (int64_t)w * 64 + lane;
            part_c[at] = ac[j];
            if (PATIENT) part_p[at] = ap[j];
        }
    }
}

// out[g * U + u] = sum_s part[(s * U + u) * GP + g], slices in order; blockIdx.y = 0 control, 1 patient
__global__ __launch_bounds__(256) void member_fold(const double *__restrict__ part_c, const double *__restrict__ part_p, int S, int U,
                                                   int64_t G, int64_t GP, double *__restrict__ out_c, double *__restrict__ out_p) {
    const double *part = blockIdx.y ? part_p : part_c;
    double *out = blockIdx.y ? out_p : out_c;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n = (int64_t)U * G;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t u = i / G, g = i - u * G;
        double v = 0.0;
        for (int s = 0; s < S; ++s) v += part[((int64_t)s * U + u) * GP + g];
        out[g * U + u] = v;
    }
}

}  // namespace

extern "C" int fcd_member_loglik(fcd_ctx *ctx, const double *x, const double *theta, const uint8_t *f_state, const uint64_t *r_bits,
                                 int64_t Nreg, int64_t U, int64_t G, int r_cols, int flags, double *out_control, double *out_patient,
                                 fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!x || !theta || !f_state || !out_control) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_member_loglik: null pointer");
    if (flags & ~FCD_DATA_NAN_MISSING) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_member_loglik: unknown flags 0x%x", flags);
    if (r_cols != 1 && r_cols != U) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_member_loglik: r_cols = %lld, must be 1 or U = %lld", r_cols, U);
    if (out_patient && !r_bits) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_member_loglik: the patient side needs r_bits");
    if (out_patient == out_control) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_member_loglik: out_patient must not alias out_control");
    LikTheta th;
    lik_theta_make(theta, th);
    // slices of the edges: two workgroups per CU whatever G is, from the shape and the device alone
    const int64_t UT = (U + MB_TU - 1) / MB_TU;
    int64_t S = (2 * (int64_t)ctx->num_cu + UT - 1) / UT;
    const int64_t s_edges = (g.C + MB_MIN_EDGES - 1) / MB_MIN_EDGES;
    if (S > s_edges) S = s_edges;
    if (S < 1) S = 1;
    if (S * UT > (1ll << 31) - 1) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_member_loglik: U=%lld exceeds the grid", U);
    const int64_t GP = (int64_t)g.GW * 64;
    const size_t n_part = (size_t)S * (size_t)U * (size_t)GP;
    rc = fcd_ws_reserve(ctx, n_part * sizeof(double) * (out_patient ? 2 : 1));
    if (rc) return rc;
    double *part_c = (double *)ctx->ws.p, *part_p = out_patient ? part_c + n_part : nullptr;
    const LikTabs *tabs = reinterpret_cast<const LikTabs *>(ctx->log_tab);
    const int missing = (flags & FCD_DATA_NAN_MISSING) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(S * UT), (unsigned)((g.GW + MB_NW - 1) / MB_NW)), block(64 * MB_NW);
#define FCD_MEMBER_LAUNCH(B, P)                                                                                              \
    hipLaunchKernelGGL((member_kernel<B, P>), grid, block, 0, s, x, th, tabs, f_state, r_bits, (int)Nreg, (int)U, g.C, g.GW, \
                       (int)S, (int)UT, missing, part_c, part_p)
    if (!out_patient)
        FCD_MEMBER_LAUNCH(true, false);
    else if (r_cols == 1)
        FCD_MEMBER_LAUNCH(true, true);
    else
        FCD_MEMBER_LAUNCH(false, true);
#undef FCD_MEMBER_LAUNCH
    FCD_LAUNCH_CHECK();
    int64_t blocks = (U * G + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cu * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(member_fold, dim3((unsigned)blocks, out_patient ? 2u : 1u), dim3(256), 0, s, (const double *)part_c,
                       (const double *)part_p, (int)S, (int)U, G, GP, out_control, out_patient);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
