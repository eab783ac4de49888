// Anomalies against an ordered patient trait: for every trait q (symptom severity, illness duration, dose ...) and every row
// rho -- a region n, or with region sets a set S ("patient u has an anomalous region in S"), the rows of
// fcd_patient_groups.hip -- the law of the rank-sum (Mann-Whitney) statistic between the patients that are anomalous at the
// row and those that are not.  The host hands every trait over as doubled, centred midranks a_u = 2 midrank_u - (n_q + 1) of
// its n_q known patients (integers, sum 0; 0 and outside `known` for the others), so a chain state gives two integers per
// (q, rho):
//     k = #{u known : the row's indicator is 1 in u},      A = sum_{u known, indicator 1} a_u
// and, where 0 < k < n_q,  AUC = 1/2 + A / (2 k (n_q - k)),  A + k (n_q - k) = 2 U_stat >= 0.  The patients are coupled
// through f, so the law of (k, A) does not follow from the per-patient marginals; only the sampler's chains carry it.
// The traits live on the context (fcd_patient_traits_set: checked on the host, so no index a kernel makes can be out of
// range).  Kernels, from the parts of fcd_tally.h as those of fcd_patient_groups.hip:
//   patient_trait_sums_kernel   one workgroup per (chain word w, row rho): the row's U words are staged in LDS, lane c is chain
//                               c and walks the patients with broadcast LDS reads; (uint16 k, int32 A) per (q, rho, chain) go
//                               to the context's scratch.
//   patient_trait_hist_kernel   one workgroup per (q, rho): the row's bins (uint32) and sums (64-bit) in LDS, the row updated
//                               once without global atomics.
#include <stdlib.h>

#include "fcd_tally.h"

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_WAVES = PT_THREADS / 64;
constexpr int PT_MAX_U = 512;
constexpr int PT_MAX_TRAITS = 16;
constexpr int PT_NB = 128;                       // AUC bins of width 1/128

__host__ __device__ inline int pt_u8(int U) { return (U + 7) & ~7; }

// Phase 1.  Grid-stride over the pairs (rho, w), w fastest; blockDim = PT_THREADS; dynamic LDS: Q * U8 int32, U8 = U rounded up
// to a multiple of 8 (the walk is unrolled by 8).
//   all threads   once: sk[q][u] = enc[q][u] = 2 a_u + known_u, ZERO for U <= u < U8.
//   all threads   stage the row (tally_stage_row): whole 64-patient chunks, zero past U.
//   wave v        traits v, v + 4, ...: lane c takes bit c of roww[u] and the trait's word of u (both broadcast reads) and adds
//                 the known bit to k, the score to A.  No transpose.
// ks, As: (Q * R) rows of GP = GW * 64 values, row q * R + rho, chain-major; chains beyond G hold whatever their bits give.
__global__ __launch_bounds__(PT_THREADS) void patient_trait_sums_kernel(const uint64_t *__restrict__ r_bits,
                                                                        const int32_t *__restrict__ rs_offsets,
                                                                        const int32_t *__restrict__ rs_members,
                                                                        const int32_t *__restrict__ enc, int Q, int Nreg, int R,
                                                                        int U, int GW, uint16_t *__restrict__ ks,
                                                                        int32_t *__restrict__ As) {
    __shared__ uint64_t roww[PT_MAX_U];
    extern __shared__ int32_t sk[];              // [Q][U8]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int U8 = pt_u8(U);
    const int64_t GP = (int64_t)GW * 64;
    const int64_t npairs = (int64_t)R * GW;
    for (int i = tid; i < Q * U8; i += PT_THREADS) {
        const int q = i / U8, u = i - q * U8;
        sk[i] = u < U ? enc[q * U + u] : 0;
    }
    // (read only after the first barrier below: the grid never exceeds the number of pairs)
    for (int64_t p = blockIdx.x; p < npairs; p += gridDim.x) {
        const int rho = (int)(p / GW), w = (int)(p % GW);
        tally_stage_row<PT_THREADS>(r_bits + (int64_t)w * Nreg * U, rs_offsets, rs_members, rho, Nreg, U, roww);
        __syncthreads();
        for (int q = wave; q < Q; q += PT_WAVES) {
            const int32_t *s = sk + q * U8;
            int k = 0, A = 0;
#pragma unroll 8
            for (int u = 0; u < U8; ++u) {
                const int bit = (int)((roww[u] >> lane) & 1ull);
                const int e = s[u];
                k += bit & e;                        // (the low bit: known)
                A += (e >> 1) & -bit;                // (arithmetic shift: the score)
            }
            const int64_t at = ((int64_t)q * R + rho) * GP + (int64_t)w * 64 + lane;
            ks[at] = (uint16_t)k;
            As[at] = A;
        }
        __syncthreads();                             // the row is read before the next pair stages its own
    }
}

// Phase 2.  Grid-stride over the rows (q, rho), one workgroup per row at a time; dynamic LDS: Umax + 1 64-bit sums, then
// W = Umax + 1 + PT_NB + 3 uint32 bins.  Only the chains g < G are binned (LDS atomics, 64-bit for the sums: integer adds, any
// order gives the same totals); both are then added to the row in place: the row belongs to this workgroup alone.
//   bins[0 .. n_q]                      k                           sums[k] += A
//   bins[Umax+1 .. Umax+PT_NB]          min(PT_NB - 1, floor(PT_NB (A + d) / (2 d))), d = k (n_q - k), where 0 < k < n_q
//   bins[Umax+1+PT_NB ..]               A < 0, A = 0, A > 0 of the same states
__global__ __launch_bounds__(256) void patient_trait_hist_kernel(const uint16_t *__restrict__ ks, const int32_t *__restrict__ As,
                                                                 const int32_t *__restrict__ nq, int QR, int R, int Umax, int GW,
                                                                 int64_t G, uint32_t *__restrict__ trait_hist,
                                                                 long long *__restrict__ trait_sum) {
    extern __shared__ unsigned long long pt_lds[];
    unsigned long long *sums = pt_lds;                               // [Umax + 1]
    uint32_t *bins = (uint32_t *)(pt_lds + Umax + 1);                // [W]
    const int tid = threadIdx.x;
    const int W = Umax + 1 + PT_NB + 3;
    const int64_t GP = (int64_t)GW * 64;
    for (int row = blockIdx.x; row < QR; row += gridDim.x) {
        const int n = nq[row / R];
        const uint16_t *sk = ks + (int64_t)row * GP;
        const int32_t *sa = As + (int64_t)row * GP;
        tally_bins_clear(bins, W);
        for (int i = tid; i <= Umax; i += blockDim.x) sums[i] = 0;
        __syncthreads();
        for (int64_t g = tid; g < G; g += blockDim.x) {
            const int k = min((int)sk[g], n);
            const int A = sa[g];
            atomicAdd(&bins[k], 1u);
            if (A) atomicAdd(&sums[k], (unsigned long long)(long long)A);     // (two's complement: the sum of signed terms)
            if (k > 0 && k < n) {
                const int d = k * (n - k);                            // <= 65536
                const int num = min(max(A + d, 0), 2 * d);            // 2 U_stat, inside [0, 2 d] by construction
                const int b = min(PT_NB - 1, (PT_NB * num) / (2 * d));
                atomicAdd(&bins[Umax + 1 + b], 1u);
                atomicAdd(&bins[Umax + 1 + PT_NB + (A < 0 ? 0 : (A == 0 ? 1 : 2))], 1u);
            }
        }
        __syncthreads();
        tally_bins_flush(bins, W, trait_hist + (int64_t)row * W);   // (bins n_q < i <= Umax stay 0: never touched)
        long long *outs = trait_sum + (int64_t)row * (Umax + 1);
        for (int i = tid; i <= Umax; i += blockDim.x) {
            const long long v = (long long)sums[i];
            if (v) outs[i] += v;
        }
        __syncthreads();                                              // read before the next row clears them
    }
}

// the refusals the tally, the accumulator and the scratch reservation share: no traits, traits made for another number of
// patients; with set rows, what tally_set_rows_check refuses
int shape_check(fcd_ctx *ctx, int64_t Nreg, int64_t U, const char *who) {
    if (ctx->pt_Q < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "no patient traits (fcd_patient_traits_set)");
    if (U != ctx->pt_U) return fcd_fail_who(ctx, FCD_ERR_SHAPE, who, "the traits were set for %lld patients, not U=%lld", ctx->pt_U, U);
    return tally_set_rows_check(ctx, Nreg, ctx->pt_with_rs, who, "traits");
}

}  // namespace

// (the caller has run shape_check)  Q R rows of GP uint16, then as many of int32
int fcd_patient_trait_ws_reserve(fcd_ctx *ctx, int64_t Nreg, int64_t, int64_t G) {
    const int64_t R = tally_rows(ctx, Nreg, ctx->pt_with_rs);
    return tally_ws_reserve(ctx, ctx->pt_Q * R, G, sizeof(uint16_t) + sizeof(int32_t),
                            "patient traits: %lld traits x %lld rows need more than 1 GiB of scratch", ctx->pt_Q, R);
}

// (the caller has checked the traits against the shape: shape_check)
int fcd_patient_trait_tally_launch(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, const fcd_geo &g,
                                   uint32_t *trait_hist, int64_t *trait_sum, hipStream_t s) {
    int rc = fcd_patient_trait_ws_reserve(ctx, Nreg, U, G); // (no-op when fcd_gibbs_run has grown it)
    if (rc) return rc;
    const int Q = (int)ctx->pt_Q, R = (int)tally_rows(ctx, Nreg, ctx->pt_with_rs), Umax = (int)ctx->pt_umax;
    const int64_t GP = (int64_t)g.GW * 64;
    uint16_t *ks = (uint16_t *)ctx->count_ws.p;
    int32_t *As = (int32_t *)(ks + (int64_t)Q * R * GP);    // (GP is a multiple of 64: aligned)
    const int32_t *enc = (const int32_t *)ctx->pt_dev, *nq = enc + (int64_t)Q * U;
    const int32_t *rs_offsets = ctx->pt_with_rs ? (const int32_t *)ctx->rs_dev : nullptr;
    const int32_t *rs_members = ctx->pt_with_rs ? rs_offsets + ctx->rs_J + 1 : nullptr;
    hipLaunchKernelGGL(patient_trait_sums_kernel, dim3(tally_grid(ctx, (int64_t)R * g.GW)), dim3(PT_THREADS),
                       (size_t)Q * pt_u8((int)U) * sizeof(int32_t), s, r_bits, rs_offsets, rs_members, enc, Q, (int)Nreg, R, (int)U, g.GW,
                       ks, As);
    FCD_LAUNCH_CHECK();
    const size_t shmem = (size_t)(Umax + 1) * sizeof(unsigned long long) + (size_t)(Umax + 1 + PT_NB + 3) * sizeof(uint32_t);
    hipLaunchKernelGGL(patient_trait_hist_kernel, dim3(tally_grid(ctx, (int64_t)Q * R)), dim3(256), shmem, s, ks, As, nq, Q * R, R, Umax,
                       g.GW, G, trait_hist, (long long *)trait_sum);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_patient_traits_set(fcd_ctx *ctx, const int32_t *scores_host, const uint8_t *known_host, int64_t Q, int64_t U,
                                      int with_region_sets) {
    static const char *who = "fcd_patient_traits_set";
    if (!ctx) return FCD_ERR_ARG;
    if (ctx->sweep_acc[FCD_ACC_PATIENT_TRAIT].buf[0]) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "the patient-trait accumulator is attached");
    if (Q == 0 && !scores_host && !known_host) {
        (void)tally_table_replace(ctx, &ctx->pt_dev, nullptr, 0);
        ctx->pt_Q = ctx->pt_U = ctx->pt_umax = 0;
        ctx->pt_with_rs = 0;
        return FCD_OK;
    }
    if (!scores_host || !known_host) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    if (Q < 1 || U < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "Q=%lld U=%lld", Q, U);
    if (Q > PT_MAX_TRAITS) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "Q=%lld (at most 16 traits)", Q);
    if (U > PT_MAX_U) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "U=%lld (at most 512 patients)", U);
    const size_t words = (size_t)(Q * U + Q);
    int32_t *host = (int32_t *)calloc(words, sizeof(int32_t));      // enc (Q, U) | n_q (Q)
    if (!host) return (int)hipErrorOutOfMemory;
    int64_t umax = 0;
    int rc = FCD_OK;
    for (int64_t q = 0; q < Q && !rc; ++q) {
        int64_t n = 0, sum = 0;
        for (int64_t u = 0; u < U; ++u) n += known_host[q * U + u] ? 1 : 0;
        if (n < 2) {
            rc = fcd_fail_who(ctx, FCD_ERR_ARG, who, "trait %lld is known for %lld patients (at least 2)", q, n);
            break;
        }
        bool distinct = false;
        for (int64_t u = 0; u < U; ++u) {
            const int64_t a = scores_host[q * U + u];
            const bool kn = known_host[q * U + u] != 0;
            if (!kn && a != 0) {
                rc = fcd_fail_who(ctx, FCD_ERR_ARG, who, "trait %lld has a score where it is not known (patient %lld)", q, u);
                break;
            }
            if (a > n - 1 || a < -(n - 1)) {
                rc = fcd_fail_who(ctx, FCD_ERR_ARG, who, "trait %lld has a score beyond n_q - 1 = %lld", q, n - 1);
                break;
            }
            if (kn && a != 0) distinct = true;               // (the sum is 0: one non-zero score means two distinct ones)
            sum += a;
            host[q * U + u] = (int32_t)(a * 2 + (kn ? 1 : 0));
        }
        if (rc) break;
        if (sum != 0) rc = fcd_fail_who(ctx, FCD_ERR_ARG, who, "the scores of trait %lld sum to %lld, not 0", q, sum);
        else if (!distinct) rc = fcd_fail_who(ctx, FCD_ERR_ARG, who, "the known patients of trait %lld all have one score", q);
        host[Q * U + q] = (int32_t)n;
        if (n > umax) umax = n;
    }
    if (!rc) rc = tally_table_replace(ctx, &ctx->pt_dev, host, words * sizeof(int32_t));
    free(host);
    if (rc) return rc;
    ctx->pt_Q = Q;
    ctx->pt_U = U;
    ctx->pt_umax = umax;
    ctx->pt_with_rs = with_region_sets ? 1 : 0;
    return FCD_OK;
}

extern "C" int fcd_gibbs_patient_trait_tally(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                                             uint32_t *trait_hist, int64_t *trait_sum, fcd_stream stream) {
    static const char *who = "fcd_gibbs_patient_trait_tally";
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!r_bits || !trait_hist || !trait_sum) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    rc = shape_check(ctx, Nreg, U, who);
    if (rc) return rc;
    return fcd_patient_trait_tally_launch(ctx, r_bits, Nreg, U, G, g, trait_hist, trait_sum, (hipStream_t)stream);
}

extern "C" int fcd_gibbs_set_patient_trait_accumulator(fcd_ctx *ctx, uint32_t *trait_hist, int64_t *trait_sum, int64_t Nreg,
                                                       int64_t U, int64_t every) {
    if (!ctx) return FCD_ERR_ARG;
    if (trait_hist && trait_sum && Nreg >= 2 && U >= 1) {    // (what fcd_sweep_acc_set refuses, it refuses first)
        int rc = shape_check(ctx, Nreg, U, "fcd_gibbs_set_patient_trait_accumulator");
        if (rc) return rc;
    }
    // (the slot's second word pointer carries the int64 buffer)
    return fcd_sweep_acc_set(ctx, FCD_ACC_PATIENT_TRAIT, trait_hist, (uint32_t *)trait_sum, Nreg, U, every,
                             "fcd_gibbs_set_patient_trait_accumulator: trait_hist and trait_sum go together",
                             "fcd_gibbs_set_patient_trait_accumulator: Nreg=%lld U=%lld", nullptr,
                             "fcd_gibbs_set_patient_trait_accumulator: every=%lld must be >= 1");
}
