// Anomalous-region counts: the law of sum_n r_nu (how many regions of patient u are anomalous) and of sum_u r_nu (in how
// many patients region n is anomalous).
//
// The IAR model shares no anomalous region between patients (doc/methods.rst, "Individual Anomalous Regions"), and inside
// one patient the r_nu are coupled through the mixture cases of their edges: these counts depend on the joint law of the
// sites, which only the sampler's chains carry.  Kernels:
//   count_sums_kernel         per-chain sum_n r_nu and sum_u r_nu of one state, both from ONE read of r_bits, into a
//                             uint16 scratch of the context.  One workgroup per chain word: a tile of rows of that word is
//                             staged in LDS; thread u adds its column into bit-sliced (vertical) counters, one per chain;
//                             wave j takes row n of the tile with lane = chain.
//   count_hist_kernel         hist_patient[u][k] += #{chains with sum_n r_nu = k}, hist_region[n][k] += #{chains with
//                             sum_u r_nu = k}: one workgroup per row, bins in LDS, the row updated once without atomics.
//   poisson_binomial_kernel   the mean-field law of the same counts under q_R (sites independent: Poisson-binomial), the
//                             exact fp64 convolution recursion, one workgroup per row.
#include "fcd_tally.h"

namespace {

constexpr int CNT_THREADS = 512;        // the column sums give every patient a thread of its own: U <= 512
constexpr int CNT_PLANES = 10;          // bit planes of the vertical counters: sums up to 1023, Nreg <= 1023
constexpr int CNT_TILE_WORDS = 4096;    // r words of one chain word staged in LDS at a time (32 KiB, 8 per thread)
constexpr int CNT_MAX_U = CNT_THREADS;
constexpr int CNT_MAX_NREG = (1 << CNT_PLANES) - 1;

constexpr int PB_THREADS = 256;
constexpr int PB_MAXK = 16;             // bins per thread: rows of up to PB_THREADS * PB_MAXK = 4096 bins
constexpr int PB_MAX_SITES = PB_THREADS * PB_MAXK - 1;

// Phase 1.  Grid-stride over chain words w.  Per tile of tn rows (n0 .. n0 + rows) of word w, staged with all threads' loads
// in flight together:
//   patient role  thread u < U: carry-save adds of the tile's column u into its tally_planes; after the last tile the 64
//                 counts go to sums row u.
//   region role   wave v: rows j = v, v + nwaves, ... of the tile; lane j counts chain j's bits over u (broadcast LDS
//                 reads) and writes it to sums row U + n0 + j (64 lanes, one 128-byte line).
// sums: (U + Nreg) rows of GP = GW * 64 uint16, chain-major within a row; chains beyond G hold whatever their bits give.
__global__ __launch_bounds__(CNT_THREADS) void count_sums_kernel(const uint64_t *__restrict__ r_bits, int Nreg, int U, int GW,
                                                                 int tn, uint16_t *__restrict__ sums) {
    extern __shared__ uint64_t tile[];           // [tn][U]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int64_t GP = (int64_t)GW * 64;
    for (int w = blockIdx.x; w < GW; w += gridDim.x) {
        const uint64_t *rw = r_bits + (int64_t)w * Nreg * U;
        tally_planes<CNT_PLANES> pl;
        pl.clear();
        for (int n0 = 0; n0 < Nreg; n0 += tn) {
            const int rows = min(tn, Nreg - n0);
            const int nw = rows * U;                 // <= CNT_TILE_WORDS: contiguous in r_bits ([w][n][u])
            const uint64_t *src = rw + (int64_t)n0 * U;
            uint64_t v[CNT_TILE_WORDS / CNT_THREADS];
#pragma unroll
            for (int q = 0; q < CNT_TILE_WORDS / CNT_THREADS; ++q) {
                const int i = q * CNT_THREADS + tid;
                v[q] = i < nw ? src[i] : 0ull;
            }
            __syncthreads();                         // the previous tile is read
#pragma unroll
            for (int q = 0; q < CNT_TILE_WORDS / CNT_THREADS; ++q) {
                const int i = q * CNT_THREADS + tid;
                if (i < nw) tile[i] = v[q];
            }
            __syncthreads();
            if (tid < U) {
                for (int j = 0; j < rows; ++j) pl.add(tile[j * U + tid]);
            }
            for (int j = wave; j < rows; j += nwaves) {
                const uint64_t *row = tile + j * U;
                int cnt = 0;
#pragma unroll 8
                for (int u = 0; u < U; ++u) cnt += (int)((row[u] >> lane) & 1ull);
                sums[(int64_t)(U + n0 + j) * GP + (int64_t)w * 64 + lane] = (uint16_t)cnt;
            }
        }
        if (tid < U) pl.store16(sums + (int64_t)tid * GP + (int64_t)w * 64);
    }
}

// Phase 2.  One workgroup per histogram row: rows 0 .. U-1 patient u (bins 0 .. Nreg), rows U .. U+Nreg-1 region n (bins
// 0 .. U), binned by tally_bin_row.
__global__ __launch_bounds__(256) void count_hist_kernel(const uint16_t *__restrict__ sums, int Nreg, int U, int GW, int64_t G,
                                                         uint32_t *__restrict__ hist_p, uint32_t *__restrict__ hist_r) {
    extern __shared__ uint32_t bins[];           // [L + 1]
    const int row = blockIdx.x;
    const bool patient = row < U;
    uint32_t *out = patient ? hist_p + (int64_t)row * (Nreg + 1) : hist_r + (int64_t)(row - U) * (U + 1);
    tally_bin_row(sums + (int64_t)row * GW * 64, G, patient ? Nreg : U, bins, out);
}

// Rows 0 .. U-1: patient u over the sites n = 0 .. Nreg-1; rows U .. U+Nreg-1: region n over u = 0 .. U-1.
// q0 = P(r = 0), q1 = P(r = 1) from lq_R (tally_q).  P[k+1] = P(count = k) with P[0] = 0; each site is one step
//   P'(k) = P(k) q0 + P(k-1) q1
// over the bins that can be non-zero, all threads reading before any writes.  Point masses stay exact at q in {0, 1}.
__global__ __launch_bounds__(PB_THREADS) void poisson_binomial_kernel(const double *__restrict__ lq_R, int Nreg, int U,
                                                                      double *__restrict__ p_patient,
                                                                      double *__restrict__ p_region) {
    extern __shared__ double sm[];               // P[L + 2], q0[PB_THREADS], q1[PB_THREADS]
    const int tid = threadIdx.x;
    const int row = blockIdx.x;
    const bool patient = row < U;
    const int L = patient ? Nreg : U;
    const int64_t site0 = patient ? (int64_t)row : (int64_t)(row - U) * U;     // index of site 0 in (Nreg, U)
    const int64_t step = patient ? U : 1;
    double *out = patient ? p_patient + (int64_t)row * (Nreg + 1) : p_region + (int64_t)(row - U) * (U + 1);
    double *P = sm, *q0 = sm + (L + 2), *q1 = q0 + PB_THREADS;
    for (int k = tid; k < L + 2; k += PB_THREADS) P[k] = (k == 1) ? 1.0 : 0.0;
    for (int i0 = 0; i0 < L; i0 += PB_THREADS) {
        __syncthreads();                         // the previous chunk of q is used (and P is initialised)
        const int i = i0 + tid;
        if (i < L) tally_q(lq_R, site0 + (int64_t)i * step, q0[tid], q1[tid]);
        __syncthreads();
        const int ni = min(PB_THREADS, L - i0);
        for (int j = 0; j < ni; ++j) {
            const double a = q0[j], b = q1[j];
            const int kmax = i0 + j + 1;         // counts 0 .. kmax after this site
            double nv[PB_MAXK];
#pragma unroll
            for (int t = 0; t < PB_MAXK; ++t) {
                const int k = tid + t * PB_THREADS;
                nv[t] = (k <= kmax) ? P[k + 1] * a + P[k] * b : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < PB_MAXK; ++t) {
                const int k = tid + t * PB_THREADS;
                if (k <= kmax) P[k + 1] = nv[t];
            }
            __syncthreads();
        }
    }
    for (int k = tid; k <= L; k += PB_THREADS) out[k] = P[k + 1];
}

}  // namespace

int fcd_count_ws_reserve(fcd_ctx *ctx, int64_t Nreg, int64_t U, int64_t G) {
    return tally_ws_reserve(ctx, Nreg + U, G, sizeof(uint16_t));
}

int fcd_count_tally_launch(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, const fcd_geo &g,
                           uint32_t *hist_patient, uint32_t *hist_region, hipStream_t s) {
    if (Nreg > CNT_MAX_NREG || U > CNT_MAX_U)
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "anomalous-region counts: Nreg=%lld U=%lld (at most 1023 regions, 512 patients)",
                        Nreg, U);
    int rc = fcd_count_ws_reserve(ctx, Nreg, U, G);         // (no-op when fcd_gibbs_run has grown it)
    if (rc) return rc;
    uint16_t *sums = (uint16_t *)ctx->count_ws.p;
    int64_t tn = CNT_TILE_WORDS / U;
    if (tn > Nreg) tn = Nreg;
    hipLaunchKernelGGL(count_sums_kernel, dim3(tally_grid(ctx, g.GW)), dim3(CNT_THREADS), (size_t)(tn * U) * sizeof(uint64_t), s,
                       r_bits, (int)Nreg, (int)U, g.GW, (int)tn, sums);
    FCD_LAUNCH_CHECK();
    const int64_t L = Nreg > U ? Nreg : U;
    hipLaunchKernelGGL(count_hist_kernel, dim3((unsigned)(U + Nreg)), dim3(256), (size_t)(L + 1) * sizeof(uint32_t), s, sums,
                       (int)Nreg, (int)U, g.GW, G, hist_patient, hist_region);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_gibbs_count_tally(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                                     uint32_t *hist_patient, uint32_t *hist_region, fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!r_bits || !hist_patient || !hist_region) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_count_tally: null pointer");
    return fcd_count_tally_launch(ctx, r_bits, Nreg, U, G, g, hist_patient, hist_region, (hipStream_t)stream);
}

extern "C" int fcd_gibbs_set_count_accumulator(fcd_ctx *ctx, uint32_t *hist_patient, uint32_t *hist_region, int64_t Nreg,
                                               int64_t U, int64_t every) {
    const bool over = Nreg > CNT_MAX_NREG || U > CNT_MAX_U;
    return fcd_sweep_acc_set(ctx, FCD_ACC_COUNT, hist_patient, hist_region, Nreg, U, every,
                             "fcd_gibbs_set_count_accumulator: hist_patient and hist_region go together",
                             "fcd_gibbs_set_count_accumulator: Nreg=%lld U=%lld",
                             over ? "fcd_gibbs_set_count_accumulator: Nreg=%lld U=%lld (at most 1023 regions, 512 patients)" : nullptr,
                             "fcd_gibbs_set_count_accumulator: every=%lld must be >= 1");
}

extern "C" int fcd_vb_count_posterior(fcd_ctx *ctx, const double *lq_R, int64_t Nreg, int64_t U, double *p_patient,
                                      double *p_region, fcd_stream stream) {
    if (!ctx) return FCD_ERR_ARG;
    if (!lq_R || !p_patient || !p_region) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_vb_count_posterior: null pointer");
    if (Nreg < 1 || U < 1) return fcd_fail(ctx, FCD_ERR_SHAPE, "fcd_vb_count_posterior: Nreg=%lld U=%lld", Nreg, U);
    if (Nreg > PB_MAX_SITES || U > PB_MAX_SITES)
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_vb_count_posterior: Nreg=%lld U=%lld (at most 4095 each)", Nreg, U);
    const int64_t L = Nreg > U ? Nreg : U;
    const size_t shmem = (size_t)(L + 2 + 2 * PB_THREADS) * sizeof(double);
    hipLaunchKernelGGL(poisson_binomial_kernel, dim3((unsigned)(U + Nreg)), dim3(PB_THREADS), shmem, (hipStream_t)stream, lq_R,
                       (int)Nreg, (int)U, p_patient, p_region);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
