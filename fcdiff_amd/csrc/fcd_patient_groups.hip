// Anomaly prevalence over user-given groups of patients, and contrasts between two groups: for every group g_j and every row
// rho -- a region n, or with region sets a set S ("patient u has an anomalous region in S") -- the law of
// k_j = #{u in g_j : the row's indicator is 1 in u}, and for every contrast (a, b) of two disjoint groups the JOINT law of
// (k_a, k_b).  The patients are coupled through f, so neither follows from the per-patient marginals; only the sampler's
// chains carry them.  fcd_region_sets.hip put sets on the region axis, this file puts them on the patient axis: the group of
// all patients at a region row gives hist_region of fcd_count.hip, at a set row hist_prev of fcd_region_sets.hip.
// The groups live on the context (fcd_patient_groups_set: CSR, checked on the host, so no index a kernel reads can be out of
// range; the device copy holds a bit mask over u per group beside the CSR).  Kernels, from the parts of fcd_tally.h:
//   patient_group_sums_kernel   one workgroup per (chain word w, row rho): the row's U words are staged in LDS, lane c gathers
//                               chain c's bit of every 64-patient chunk into one word, and the count of group j is the
//                               popcount of that word under the group's mask; 64 counts per (j, rho, w) go as uint16 to the
//                               context's scratch.
//   patient_group_hist_kernel   one workgroup per histogram row ((j, rho) of hist_group, (p, rho) of hist_joint): bins in LDS,
//                               the row updated once without atomics.
#include <stdlib.h>

#include "fcd_tally.h"

namespace {

constexpr int PG_THREADS = 256;
constexpr int PG_WAVES = PG_THREADS / 64;
constexpr int PG_MAX_U = 512;
constexpr int PG_WORDS = PG_MAX_U / 64;         // mask words per group: the kernel reads the first ceil(U/64)
constexpr int PG_MAX_GROUPS = 64;
constexpr int PG_MAX_CONTRASTS = 64;
constexpr int PG_MAX_BINS = 16384;              // (|a|+1)(|b|+1) of a contrast: 64 KiB of uint32, the LDS of one workgroup

// Phase 1.  Grid-stride over the pairs (rho, w), w fastest; blockDim = PG_THREADS.
//   all threads   stage the row (tally_stage_row): whole 64-patient chunks, zero past U.
//   wave v        chunks v, v + 4: lane c collects bit c of the chunk's 64 words (broadcast LDS reads) -- the 64 x 64 bit
//                 transpose, one column per lane -- into colw[chunk][c].
//   wave v        groups v, v + 4, ...: lane c adds popcount(colw[chunk][c] & mask[j][chunk]) over the chunks.
// sums: (J * R) rows of GP = GW * 64 uint16, row j * R + rho, chain-major; chains beyond G hold whatever their bits give.
__global__ __launch_bounds__(PG_THREADS) void patient_group_sums_kernel(const uint64_t *__restrict__ r_bits,
                                                                        const int32_t *__restrict__ rs_offsets,
                                                                        const int32_t *__restrict__ rs_members,
                                                                        const uint64_t *__restrict__ masks, int J, int Nreg, int R,
                                                                        int U, int GW, uint16_t *__restrict__ sums) {
    __shared__ uint64_t roww[PG_MAX_U];
    __shared__ uint64_t colw[PG_WORDS][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NC = (U + 63) / 64;
    const int64_t GP = (int64_t)GW * 64;
    const int64_t npairs = (int64_t)R * GW;
    for (int64_t p = blockIdx.x; p < npairs; p += gridDim.x) {
        const int rho = (int)(p / GW), w = (int)(p % GW);
        tally_stage_row<PG_THREADS>(r_bits + (int64_t)w * Nreg * U, rs_offsets, rs_members, rho, Nreg, U, roww);
        __syncthreads();
        for (int q = wave; q < NC; q += PG_WAVES) {
            uint64_t word = 0;
#pragma unroll 8
            for (int i = 0; i < 64; ++i) word |= ((roww[q * 64 + i] >> lane) & 1ull) << i;
            colw[q][lane] = word;
        }
        __syncthreads();                             // (also: the row is read before the next pair stages its own)
        for (int j = wave; j < J; j += PG_WAVES) {
            int cnt = 0;
            for (int q = 0; q < NC; ++q) cnt += __popcll(colw[q][lane] & masks[j * PG_WORDS + q]);
            sums[((int64_t)j * R + rho) * GP + (int64_t)w * 64 + lane] = (uint16_t)cnt;
        }
        // (colw is written again only after the next pair's first barrier, which every wave reaches after these reads)
    }
}

// Phase 2.  One workgroup per histogram row: rows 0 .. J*R-1 are (group j, row rho) with bins 0 .. |g_j| of hist_group
// (J, R, Umax+1) -- the bins beyond the group's size are never touched --, rows J*R .. J*R+P*R-1 (contrast p = (a, b), row rho)
// with the (|a|+1)(|b|+1) bins k_a * (|b|+1) + k_b of hist_joint, whose block p starts at R * boff[p].  Both are binned in LDS
// and added in place as tally_bin_row does, from its two halves: each kind of row has its binning rule, and ONE flush serves
// both (the whole-row helper in the first branch makes a second copy of the flush, measured 1 % on a tally).  Only the chains
// g < G are binned.
__global__ __launch_bounds__(256) void patient_group_hist_kernel(const uint16_t *__restrict__ sums,
                                                                 const int32_t *__restrict__ offsets,
                                                                 const int32_t *__restrict__ contrasts,
                                                                 const int64_t *__restrict__ boff, int J, int R, int Umax, int GW,
                                                                 int64_t G, uint32_t *__restrict__ hist_group,
                                                                 uint32_t *__restrict__ hist_joint) {
    extern __shared__ uint32_t bins[];           // [max(Umax + 1, largest contrast)]
    const int row = blockIdx.x, tid = threadIdx.x;
    const int64_t GP = (int64_t)GW * 64;
    int nb;
    uint32_t *out;
    if (row < J * R) {
        const int j = row / R;
        const int L = offsets[j + 1] - offsets[j];
        nb = L + 1;
        out = hist_group + (int64_t)row * (Umax + 1);
        const uint16_t *src = sums + (int64_t)row * GP;
        tally_bins_clear(bins, nb);
        __syncthreads();
        for (int64_t g = tid; g < G; g += blockDim.x) atomicAdd(&bins[min((int)src[g], L)], 1u);
    } else {
        const int q = row - J * R, p = q / R, rho = q % R;
        const int a = contrasts[2 * p], b = contrasts[2 * p + 1];
        const int La = offsets[a + 1] - offsets[a], Lb = offsets[b + 1] - offsets[b];
        nb = (La + 1) * (Lb + 1);
        out = hist_joint + boff[p] * R + (int64_t)rho * nb;
        const uint16_t *sa = sums + ((int64_t)a * R + rho) * GP, *sb = sums + ((int64_t)b * R + rho) * GP;
        tally_bins_clear(bins, nb);
        __syncthreads();
        for (int64_t g = tid; g < G; g += blockDim.x)
            atomicAdd(&bins[min((int)sa[g], La) * (Lb + 1) + min((int)sb[g], Lb)], 1u);
    }
    __syncthreads();
    tally_bins_flush(bins, nb, out);
}

// the refusals the tally, the accumulator and the scratch reservation share: no groups, more patients than the masks hold, a
// member outside the patients; with set rows, what tally_set_rows_check refuses
int shape_check(fcd_ctx *ctx, int64_t Nreg, int64_t U, const char *who) {
    if (ctx->pg_J < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "no patient groups (fcd_patient_groups_set)");
    if (U > PG_MAX_U) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "U=%lld (at most 512 patients)", U);
    if (ctx->pg_max_member >= U)
        return fcd_fail_who(ctx, FCD_ERR_SHAPE, who, "member %lld of a patient group with U=%lld", ctx->pg_max_member, U);
    return tally_set_rows_check(ctx, Nreg, ctx->pg_with_rs, who, "groups");
}

// byte offsets inside the device copy: offsets | members | contrasts | (8-byte boundary) masks | boff
struct pg_layout {
    size_t members, contrasts, masks, boff, bytes;
};
pg_layout layout_of(int64_t J, int64_t total, int64_t P) {
    pg_layout l;
    l.members = (size_t)(J + 1) * sizeof(int32_t);
    l.contrasts = l.members + (size_t)total * sizeof(int32_t);
    l.masks = (l.contrasts + (size_t)(2 * P) * sizeof(int32_t) + 7) & ~(size_t)7;
    l.boff = l.masks + (size_t)J * PG_WORDS * sizeof(uint64_t);
    l.bytes = l.boff + (size_t)(P + 1) * sizeof(int64_t);
    return l;
}

}  // namespace

// (the caller has run shape_check)
int fcd_patient_group_ws_reserve(fcd_ctx *ctx, int64_t Nreg, int64_t, int64_t G) {
    const int64_t R = tally_rows(ctx, Nreg, ctx->pg_with_rs);
    return tally_ws_reserve(ctx, ctx->pg_J * R, G, sizeof(uint16_t),
                            "patient groups: %lld groups x %lld rows need more than 1 GiB of scratch", ctx->pg_J, R);
}

// (the caller has checked the groups against the shape: shape_check)
int fcd_patient_group_tally_launch(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, const fcd_geo &g,
                                   uint32_t *hist_group, uint32_t *hist_joint, hipStream_t s) {
    int rc = fcd_patient_group_ws_reserve(ctx, Nreg, U, G); // (no-op when fcd_gibbs_run has grown it)
    if (rc) return rc;
    uint16_t *sums = (uint16_t *)ctx->count_ws.p;
    const int J = (int)ctx->pg_J, P = (int)ctx->pg_P, R = (int)tally_rows(ctx, Nreg, ctx->pg_with_rs), Umax = (int)ctx->pg_umax;
    const pg_layout l = layout_of(J, ctx->pg_total, P);
    const char *dev = (const char *)ctx->pg_dev;
    const int32_t *offsets = (const int32_t *)dev, *contrasts = (const int32_t *)(dev + l.contrasts);
    const uint64_t *masks = (const uint64_t *)(dev + l.masks);
    const int64_t *boff = (const int64_t *)(dev + l.boff);
    const int32_t *rs_offsets = ctx->pg_with_rs ? (const int32_t *)ctx->rs_dev : nullptr;
    const int32_t *rs_members = ctx->pg_with_rs ? rs_offsets + ctx->rs_J + 1 : nullptr;
    hipLaunchKernelGGL(patient_group_sums_kernel, dim3(tally_grid(ctx, (int64_t)R * g.GW)), dim3(PG_THREADS), 0, s, r_bits, rs_offsets,
                       rs_members, masks, J, (int)Nreg, R, (int)U, g.GW, sums);
    FCD_LAUNCH_CHECK();
    const int64_t nb = ctx->pg_bins_max > Umax + 1 ? ctx->pg_bins_max : Umax + 1;
    hipLaunchKernelGGL(patient_group_hist_kernel, dim3((unsigned)((int64_t)(J + P) * R)), dim3(256), (size_t)nb * sizeof(uint32_t), s,
                       sums, offsets, contrasts, boff, J, R, Umax, g.GW, G, hist_group, hist_joint);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_patient_groups_set(fcd_ctx *ctx, const int32_t *offsets_host, const int32_t *members_host, int64_t J,
                                      const int32_t *contrasts_host, int64_t P, int with_region_sets) {
    static const char *who = "fcd_patient_groups_set";
    if (!ctx) return FCD_ERR_ARG;
    if (ctx->sweep_acc[FCD_ACC_PATIENT_GROUP].buf[0]) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "the patient-group accumulator is attached");
    const bool clear = J == 0 && !offsets_host && !members_host;
    if (clear) {
        if (P != 0 || contrasts_host) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "contrasts without groups");
        (void)tally_table_replace(ctx, &ctx->pg_dev, nullptr, 0);
        ctx->pg_J = ctx->pg_P = ctx->pg_umax = ctx->pg_total = ctx->pg_bins_max = 0;
        ctx->pg_max_member = -1;
        ctx->pg_with_rs = 0;
        return FCD_OK;
    }
    if (!offsets_host || !members_host) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    if (J < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "J=%lld", J);
    if (J > PG_MAX_GROUPS) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "J=%lld (at most 64 groups)", J);
    if (P < 0 || (P > 0 && !contrasts_host)) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "P=%lld contrasts and no array of them", P);
    if (P > PG_MAX_CONTRASTS) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "P=%lld (at most 64 contrasts)", P);
    int64_t umax = 0, max_member = -1, bins_max = 0;
    int rc = tally_csr_check([ctx](int code, const char *fmt, long long a, long long b) { return fcd_fail_who(ctx, code, who, fmt, a, b); },
                             "group", offsets_host, members_host, J, &umax, &max_member);
    if (rc) return rc;
    uint64_t masks[PG_MAX_GROUPS][PG_WORDS];
    int64_t boff[PG_MAX_CONTRASTS + 1];
    memset(masks, 0, sizeof(masks));
    for (int64_t j = 0; j < J; ++j) {
        for (int64_t i = offsets_host[j]; i < offsets_host[j + 1]; ++i) {
            const int64_t u = members_host[i];
            if (u >= PG_MAX_U) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "group %lld has the member %lld (at most 512 patients)", j, u);
            masks[j][u >> 6] |= 1ull << (u & 63);
        }
    }
    const int64_t total = offsets_host[J];
    boff[0] = 0;
    for (int64_t p = 0; p < P; ++p) {
        const int64_t a = contrasts_host[2 * p], b = contrasts_host[2 * p + 1];
        if (a < 0 || a >= J || b < 0 || b >= J) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "contrast %lld names a group outside [0, %lld)", p, J);
        if (a == b) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "contrast %lld names group %lld twice", p, a);
        for (int q = 0; q < PG_WORDS; ++q)
            if (masks[a][q] & masks[b][q]) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "the groups of contrast %lld overlap", p);
        const int64_t nb = (int64_t)(offsets_host[a + 1] - offsets_host[a] + 1) * (offsets_host[b + 1] - offsets_host[b] + 1);
        if (nb > PG_MAX_BINS) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "contrast %lld has %lld joint bins (at most 16384)", p, nb);
        if (nb > bins_max) bins_max = nb;
        boff[p + 1] = boff[p] + nb;
    }
    const pg_layout l = layout_of(J, total, P);
    char *host = (char *)calloc(1, l.bytes);
    if (!host) return (int)hipErrorOutOfMemory;
    memcpy(host, offsets_host, (size_t)(J + 1) * sizeof(int32_t));
    memcpy(host + l.members, members_host, (size_t)total * sizeof(int32_t));
    if (P) memcpy(host + l.contrasts, contrasts_host, (size_t)(2 * P) * sizeof(int32_t));
    memcpy(host + l.masks, masks, (size_t)J * PG_WORDS * sizeof(uint64_t));
    memcpy(host + l.boff, boff, (size_t)(P + 1) * sizeof(int64_t));
    rc = tally_table_replace(ctx, &ctx->pg_dev, host, l.bytes);
    free(host);
    if (rc) return rc;
    ctx->pg_J = J;
    ctx->pg_P = P;
    ctx->pg_umax = umax;
    ctx->pg_max_member = max_member;
    ctx->pg_total = total;
    ctx->pg_bins_max = bins_max;
    ctx->pg_with_rs = with_region_sets ? 1 : 0;
    return FCD_OK;
}

extern "C" int fcd_gibbs_patient_group_tally(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                                             uint32_t *hist_group, uint32_t *hist_joint, fcd_stream stream) {
    static const char *who = "fcd_gibbs_patient_group_tally";
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!r_bits || !hist_group || !hist_joint) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    rc = shape_check(ctx, Nreg, U, who);
    if (rc) return rc;
    return fcd_patient_group_tally_launch(ctx, r_bits, Nreg, U, G, g, hist_group, hist_joint, (hipStream_t)stream);
}

extern "C" int fcd_gibbs_set_patient_group_accumulator(fcd_ctx *ctx, uint32_t *hist_group, uint32_t *hist_joint, int64_t Nreg,
                                                       int64_t U, int64_t every) {
    if (!ctx) return FCD_ERR_ARG;
    if (hist_group && hist_joint && Nreg >= 2 && U >= 1) {   // (what fcd_sweep_acc_set refuses, it refuses first)
        int rc = shape_check(ctx, Nreg, U, "fcd_gibbs_set_patient_group_accumulator");
        if (rc) return rc;
    }
    return fcd_sweep_acc_set(ctx, FCD_ACC_PATIENT_GROUP, hist_group, hist_joint, Nreg, U, every,
                             "fcd_gibbs_set_patient_group_accumulator: hist_group and hist_joint go together",
                             "fcd_gibbs_set_patient_group_accumulator: Nreg=%lld U=%lld", nullptr,
                             "fcd_gibbs_set_patient_group_accumulator: every=%lld must be >= 1");
}
