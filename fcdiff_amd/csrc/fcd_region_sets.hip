// Anomalous-region counts over user-given sets of regions (networks of an atlas): for every set S_j the law of
// sum_{n in S_j} r_nu (how many regions of the set are anomalous in patient u) and of #{u : some n in S_j has r_nu = 1} (in
// how many patients the set is hit).  Like the counts of fcd_count.hip -- which these generalise: the set of all regions
// gives hist_patient, a singleton {n} gives hist_region[n] -- they depend on the joint law of the sites, which only the
// sampler's chains carry.  The sets live on the context (fcd_region_sets_set: CSR, checked on the host, so no index a
// kernel reads can be out of range).  Kernels, from the parts of fcd_tally.h as those of fcd_count.hip:
//   region_set_sums_kernel    one workgroup per (chain word w, set j): thread u adds the set's rows of column u into
//                             bit-sliced (vertical) counters, one per chain, and writes the 64 counts as uint16 to the
//                             context's scratch; the OR of the planes is the "any" word of (j, u), and one wave with
//                             lane = chain counts its bit over u.
//   region_set_hist_kernel    one workgroup per histogram row (J*U rows of hist_set, J of hist_prev): bins in LDS, the row
//                             updated once without atomics.
#include "fcd_tally.h"

namespace {

constexpr int RS_THREADS = 512;         // every patient has a thread of its own: U <= 512
constexpr int RS_PLANES = 10;           // bit planes of the vertical counters: sets of up to 1023 regions
constexpr int RS_MAX_U = RS_THREADS;
constexpr int RS_MAX_SIZE = (1 << RS_PLANES) - 1;
constexpr int RS_MAX_SETS = 1024;

// Phase 1.  Grid-stride over the pairs (j, w), w fastest.  blockDim = U rounded up to whole waves.
//   thread u < U   walks the members of S_j (the member index is uniform over the workgroup; the loads of r_bits[w][n][u] are
//                  coalesced over u), carry-save adds into its tally_planes; the 64 counts go to sums row j*U + u, the OR
//                  of the planes to LDS.
//   wave 0         lane c counts chain c's bit of the "any" words over u (broadcast LDS reads): sums row J*U + j.
// sums: (J*U + J) rows of GP = GW * 64 uint16, chain-major within a row; chains beyond G hold whatever their bits give.
__global__ __launch_bounds__(RS_THREADS) void region_set_sums_kernel(const uint64_t *__restrict__ r_bits,
                                                                     const int32_t *__restrict__ offsets,
                                                                     const int32_t *__restrict__ members, int J, int Nreg, int U,
                                                                     int GW, uint16_t *__restrict__ sums) {
    __shared__ uint64_t anyw[RS_MAX_U];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t GP = (int64_t)GW * 64;
    const int64_t npairs = (int64_t)J * GW;
    for (int64_t p = blockIdx.x; p < npairs; p += gridDim.x) {
        const int j = (int)(p / GW), w = (int)(p % GW);
        const int i0 = offsets[j], i1 = offsets[j + 1];
        if (tid < U) {
            const uint64_t *col = r_bits + (int64_t)w * Nreg * U + tid;
            tally_planes<RS_PLANES> pl;
            pl.clear();
#pragma unroll 4
            for (int i = i0; i < i1; ++i) pl.add(col[(int64_t)members[i] * U]);
            anyw[tid] = pl.any();
            pl.store16(sums + ((int64_t)j * U + tid) * GP + (int64_t)w * 64);
        }
        __syncthreads();
        if (tid < 64) {
            int cnt = 0;
#pragma unroll 8
            for (int u = 0; u < U; ++u) cnt += (int)((anyw[u] >> lane) & 1ull);
            sums[((int64_t)J * U + j) * GP + (int64_t)w * 64 + lane] = (uint16_t)cnt;
        }
        __syncthreads();                             // the "any" words are read before the next pair writes them
    }
}

// Phase 2.  One workgroup per histogram row: rows 0 .. J*U-1 are (set j, patient u) with bins 0 .. |S_j| of hist_set
// (J, U, S_max+1) -- the bins beyond the set's size are never touched --, rows J*U .. J*U+J-1 set j with bins 0 .. U of
// hist_prev (J, U+1), binned by tally_bin_row.
__global__ __launch_bounds__(256) void region_set_hist_kernel(const uint16_t *__restrict__ sums,
                                                              const int32_t *__restrict__ offsets, int J, int U, int S_max, int GW,
                                                              int64_t G, uint32_t *__restrict__ hist_set,
                                                              uint32_t *__restrict__ hist_prev) {
    extern __shared__ uint32_t bins[];           // [L + 1]
    const int row = blockIdx.x;
    const bool per_patient = row < J * U;
    const int j = per_patient ? row / U : row - J * U;
    const int L = per_patient ? offsets[j + 1] - offsets[j] : U;
    uint32_t *out = per_patient ? hist_set + (int64_t)row * (S_max + 1) : hist_prev + (int64_t)j * (U + 1);
    tally_bin_row(sums + (int64_t)row * GW * 64, G, L, bins, out);
}

// the refusals the tally and the accumulator share: no sets, a member outside the regions, more patients than threads
int shape_check(fcd_ctx *ctx, int64_t Nreg, int64_t U, const char *msg_none, const char *msg_member, const char *msg_u) {
    if (ctx->rs_J < 1) return fcd_fail(ctx, FCD_ERR_ARG, msg_none);
    if (ctx->rs_max_member >= Nreg) return fcd_fail(ctx, FCD_ERR_SHAPE, msg_member, ctx->rs_max_member, Nreg);
    if (U > RS_MAX_U) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, msg_u, U);
    return FCD_OK;
}

}  // namespace

int fcd_region_set_ws_reserve(fcd_ctx *ctx, int64_t, int64_t U, int64_t G) {
    return tally_ws_reserve(ctx, ctx->rs_J * U + ctx->rs_J, G, sizeof(uint16_t),
                            "region sets: %lld sets x %lld patients need more than 1 GiB of scratch", ctx->rs_J, U);
}

// (the caller has checked the sets against the shape: shape_check)
int fcd_region_set_tally_launch(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, const fcd_geo &g,
                                uint32_t *hist_set, uint32_t *hist_prev, hipStream_t s) {
    int rc = fcd_region_set_ws_reserve(ctx, Nreg, U, G);    // (no-op when fcd_gibbs_run has grown it)
    if (rc) return rc;
    uint16_t *sums = (uint16_t *)ctx->count_ws.p;
    const int32_t *offsets = (const int32_t *)ctx->rs_dev, *members = offsets + ctx->rs_J + 1;
    const int J = (int)ctx->rs_J, S_max = (int)ctx->rs_smax;
    const int threads = (int)((U + 63) / 64) * 64;
    hipLaunchKernelGGL(region_set_sums_kernel, dim3(tally_grid(ctx, (int64_t)J * g.GW)), dim3(threads), 0, s, r_bits, offsets, members,
                       J, (int)Nreg, (int)U, g.GW, sums);
    FCD_LAUNCH_CHECK();
    const int64_t L = S_max > U ? S_max : U;
    hipLaunchKernelGGL(region_set_hist_kernel, dim3((unsigned)(J * U + J)), dim3(256), (size_t)(L + 1) * sizeof(uint32_t), s, sums,
                       offsets, J, (int)U, S_max, g.GW, G, hist_set, hist_prev);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_region_sets_set(fcd_ctx *ctx, const int32_t *offsets_host, const int32_t *members_host, int64_t J) {
    if (!ctx) return FCD_ERR_ARG;
    if (ctx->sweep_acc[FCD_ACC_REGION_SET].buf[0])
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_region_sets_set: the region-set accumulator is attached");
    if (ctx->pg_with_rs && ctx->sweep_acc[FCD_ACC_PATIENT_GROUP].buf[0])
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_region_sets_set: the patient-group accumulator is attached with the sets as rows");
    if (ctx->pt_with_rs && ctx->sweep_acc[FCD_ACC_PATIENT_TRAIT].buf[0])
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_region_sets_set: the patient-trait accumulator is attached with the sets as rows");
    const bool clear = J == 0 && !offsets_host && !members_host;
    int64_t smax = 0, max_member = -1, total = 0;
    if (!clear) {
        if (!offsets_host || !members_host) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_region_sets_set: null pointer");
        if (J < 1) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_region_sets_set: J=%lld", J);
        if (J > RS_MAX_SETS) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_region_sets_set: J=%lld (at most 1024 sets)", J);
        const auto fail = [ctx](int code, const char *fmt, long long a, long long b) {
            return fcd_fail_who(ctx, code, "fcd_region_sets_set", fmt, a, b);
        };
        int rc = tally_csr_check(fail, "set", offsets_host, members_host, J, &smax, &max_member);
        if (rc) return rc;
        for (int64_t j = 0; j < J && smax > RS_MAX_SIZE; ++j) {
            const int64_t size = offsets_host[j + 1] - offsets_host[j];
            if (size > RS_MAX_SIZE) return fail(FCD_ERR_UNSUPPORTED, "set %lld has %lld members (at most 1023)", j, size);
        }
        total = offsets_host[J];
    }
    int rc = tally_table_replace(ctx, &ctx->rs_dev, offsets_host, clear ? 0 : (size_t)(J + 1) * sizeof(int32_t), members_host,
                                 (size_t)total * sizeof(int32_t));
    if (rc) return rc;
    ctx->rs_J = clear ? 0 : J;
    ctx->rs_smax = smax;
    ctx->rs_max_member = max_member;
    return FCD_OK;
}

extern "C" int fcd_gibbs_region_set_tally(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                                          uint32_t *hist_set, uint32_t *hist_prev, fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!r_bits || !hist_set || !hist_prev) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_region_set_tally: null pointer");
    rc = shape_check(ctx, Nreg, U, "fcd_gibbs_region_set_tally: no region sets (fcd_region_sets_set)",
                     "fcd_gibbs_region_set_tally: member %lld of a region set with Nreg=%lld",
                     "fcd_gibbs_region_set_tally: U=%lld (at most 512 patients)");
    if (rc) return rc;
    return fcd_region_set_tally_launch(ctx, r_bits, Nreg, U, G, g, hist_set, hist_prev, (hipStream_t)stream);
}

extern "C" int fcd_gibbs_set_region_set_accumulator(fcd_ctx *ctx, uint32_t *hist_set, uint32_t *hist_prev, int64_t Nreg,
                                                    int64_t U, int64_t every) {
    if (!ctx) return FCD_ERR_ARG;
    if (hist_set && hist_prev && Nreg >= 2 && U >= 1) {      // (what fcd_sweep_acc_set refuses, it refuses first)
        int rc = shape_check(ctx, Nreg, U, "fcd_gibbs_set_region_set_accumulator: no region sets (fcd_region_sets_set)",
                             "fcd_gibbs_set_region_set_accumulator: member %lld of a region set with Nreg=%lld",
                             "fcd_gibbs_set_region_set_accumulator: U=%lld (at most 512 patients)");
        if (rc) return rc;
    }
    return fcd_sweep_acc_set(ctx, FCD_ACC_REGION_SET, hist_set, hist_prev, Nreg, U, every,
                             "fcd_gibbs_set_region_set_accumulator: hist_set and hist_prev go together",
                             "fcd_gibbs_set_region_set_accumulator: Nreg=%lld U=%lld", nullptr,
                             "fcd_gibbs_set_region_set_accumulator: every=%lld must be >= 1");
}
