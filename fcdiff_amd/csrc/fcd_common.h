// Shared host/device helpers of libfcdiff_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/fcdiff_hip.h"
#include "fcd_knobs.h"

#define FCD_PROF_SLOTS 4
#define FCD_PROF_LIK 0
#define FCD_PROF_F 1
#define FCD_PROF_RSTEP 2
#define FCD_PROF_PACK 3

// kernels whose dynamic-LDS limit is raised with hipFuncSetAttribute: done once per (kernel, size) and remembered here
enum { FCD_KA_F_GENERIC = 0, FCD_KA_F_COND, FCD_KA_F_DIFF, FCD_KA_F_PAIR, FCD_KA_F_PAIR_T = FCD_KA_F_PAIR + 4,
       FCD_KA_F_PAIR_R = FCD_KA_F_PAIR_T + 4, FCD_KA_F_PAIR_S = FCD_KA_F_PAIR_R + 4,
       FCD_KA_F_PAIR_BIG = FCD_KA_F_PAIR_S + 4, FCD_KA_R_STEP = FCD_KA_F_PAIR_BIG + 4, FCD_KA_R_PIPE = FCD_KA_R_STEP + 4, FCD_KA_CORR = FCD_KA_R_PIPE + 4, FCD_KA_COMPONENTS = FCD_KA_CORR + 1,
       FCD_KA_GLM = FCD_KA_COMPONENTS + 1,      // 4 kernels (observed, permutations, bits, bits with excess) x 4 design widths
       FCD_KA_PARTIAL = FCD_KA_GLM + 16,        // fcd_corr_partial's inversion kernel
       FCD_KA_EIGH = FCD_KA_PARTIAL + 1,        // fcd_sym_eigh's Jacobi kernel
       FCD_KA_COMPONENTS_W = FCD_KA_EIGH + 1,   // fcd_graph_components_weighted's kernel
       FCD_KA_N = FCD_KA_COMPONENTS_W + 1 };

#define FCD_NAN_SLOTS 256
#define FCD_F_SLOTS 64
// bytes of the context's fixed-size device blocks (fcd_ctx::acc, f_slots, nan_slots): what is allocated is what is cleared
constexpr size_t FCD_ACC_BYTES = 8 * sizeof(unsigned long long);
constexpr size_t FCD_F_SLOTS_BYTES = FCD_F_SLOTS * 8 * sizeof(unsigned long long);
constexpr size_t FCD_NAN_SLOTS_BYTES = FCD_NAN_SLOTS * 16 * sizeof(unsigned long long);

// A device block the context owns and only ever grows (fcd_buf_reserve: drain the device, free, allocate).  min_bytes: what
// the first growth asks for at least.  zeroed / counted: the block is zero-filled when it grows / the growth adds one to
// fcd_ctx::n_alloc.  Every block is counted and left as allocated but K_corr's tickets: their kernels find them zero and
// leave them zero, so a new block must start that way, and n_alloc has never included them -- the stat is what callers
// compare across calls, so it stays that way.
struct fcd_dev_buf {
    void *p;
    size_t bytes;
    size_t min_bytes;
    bool zeroed, counted;
};

// The context's device words (fcd_ctx::words), 16 x 8 bytes: event counters read by fcd_ctx_stat under the names in quotes
// and never reset by the library, and what the kernels of one sweep-loop call hand to each other.  The offsets are fixed
// (static_asserts below): a kernel takes the block, or a pointer to one member.
struct fcd_dev_words {
    unsigned long long f_repeats;          // waves of the f pass that repeated an edge's sums in fp64 ("f_repeats")
    unsigned long long r_exact_rows;       // rows of the r pass's in-order role decided on the exact path ("r_exact_rows")
    unsigned long long f_sure_tiles;       // workgroups of the pair-tile f pass that took the decided-tile path ("f_sure_tiles")
    unsigned long long f_sure_fallbacks;   // ... decided ones its vote sent back ("f_sure_fallbacks")
    unsigned tile_decided, tile_open;      // the record build's "some tile is decided" / "some tile is open", zero between calls
    const double *lM, *hyper;              // the call's lM and hyper, for the kernels that read its record table
    unsigned long long reserved7;
    unsigned long long r_sure_sites;       // (site, chain word) items a sparse r pass left to its tables ("r_sure_sites")
    unsigned long long r_sure_exceptions;  // ... decided ones it evaluated in full all the same ("r_sure_exceptions")
    unsigned long long r_decided;          // sites the r pass's bound build found decided, zero between calls
    double hyper0[5];                      // the call's starting hyper (gibbs_f_hint_kernel: the bound build reads it there)
};
static_assert(sizeof(fcd_dev_words) == 128, "sixteen 8-byte words");
static_assert(offsetof(fcd_dev_words, f_repeats) == 0 && offsetof(fcd_dev_words, r_exact_rows) == 8 &&
                  offsetof(fcd_dev_words, f_sure_tiles) == 16 && offsetof(fcd_dev_words, f_sure_fallbacks) == 24,
              "words 0-3");
static_assert(offsetof(fcd_dev_words, tile_decided) == 32 && offsetof(fcd_dev_words, tile_open) == 36, "word 4");
static_assert(offsetof(fcd_dev_words, lM) == 40 && offsetof(fcd_dev_words, hyper) == 48 &&
                  offsetof(fcd_dev_words, reserved7) == 56,
              "words 5-7");
static_assert(offsetof(fcd_dev_words, r_sure_sites) == 64 && offsetof(fcd_dev_words, r_sure_exceptions) == 72 &&
                  offsetof(fcd_dev_words, r_decided) == 80 && offsetof(fcd_dev_words, hyper0) == 88,
              "words 8-15");

// The pinned hint words the sweep loop polls (fcd_hint_wait).  f: the records kernel of build number n_frec_build leaves four
// times that number, + 1 where some tile of its table has every edge decided (FCD_F_SURE_DRIFT nats in hand), + 2 where
// every tile has.  r: the bound build of number n_rsure_build leaves four times that number, + 1 where at least
// R_SURE_MIN_SHARE of the sites are decided, + 2 where any is.
struct fcd_hint_words {
    unsigned f, r;
};
// What the pinned error word (fcd_ctx::dev_err) carries; fcd_ctx_check turns it into a message
constexpr unsigned FCD_DEV_ERR_R_ABANDONED = 1u;   // a device-side wait of the pipelined r pass was given up
constexpr unsigned FCD_DEV_ERR_HARM_SITE = 2u;     // fcd_site_harmonize: a site id outside 0..B-1

// The optional tallies fcd_gibbs_run adds to caller-owned uint32 buffers after a counted sweep, in the order it makes them:
// (C, U, 3, 3) counts of (f_c, mixture case) (fcd_gibbs_set_pair_accumulator; one buffer, held in both places), (U, Nreg+1) /
// (Nreg, U+1) histograms of the anomalous-region counts (fcd_gibbs_set_count_accumulator), (Nreg, Nreg) / (U, U) co-anomaly
// counts (fcd_gibbs_set_coanomaly_accumulator), (J, U, S_max+1) / (J, U+1) histograms of the counts over the context's region
// sets (fcd_gibbs_set_region_set_accumulator), (J, R, Umax+1) / flat joint histograms of the counts over the context's patient
// groups and contrasts (fcd_gibbs_set_patient_group_accumulator), (Q, R, Umax+1+128+3) uint32 / (Q, R, Umax+1) int64 rank-sum
// histograms and sums over the context's patient traits (fcd_gibbs_set_patient_trait_accumulator).  fcd_gibbs.hip holds the
// launch of each.
enum { FCD_ACC_PAIR, FCD_ACC_COUNT, FCD_ACC_COANOMALY, FCD_ACC_REGION_SET, FCD_ACC_PATIENT_GROUP, FCD_ACC_PATIENT_TRAIT, FCD_ACC_N };
struct fcd_sweep_acc {
    uint32_t *buf[2];              // buf[0] == nullptr: detached (the patient-trait slot keeps its int64 buffer in buf[1])
    int64_t nreg = 0, u = 0, every = 1;    // the shape it was made for; added at every this many sweeps from accumulate_from on
};

// Everything starts at zero (fcd_ctx_create value-initialises) but the members that say otherwise.
struct fcd_ctx {
    int device;
    int num_cu;        // of the device's properties (fcd_ctx_create)
    fcd_dev_buf ws = {nullptr, 0, (size_t)1 << 20, false, true};      // reduction / partial-sum workspace
    fcd_knobs knobs;
    long long n_alloc;             // device allocations made by this context so far (fcd_ctx_stat "n_alloc")
    size_t lds_attr[FCD_KA_N];     // largest dynamic-LDS size already set per kernel
    int pipe_occ[3] = {-1, -1, -1};        // pipelined r pass: workgroups per CU of the three kernel variants (-1: not asked yet) ...
    size_t pipe_occ_shmem[3];      // ... for this much dynamic LDS
    int pipe_occ_threads[3];       // ... and this many threads
    int64_t pipe_grid;             // last pipelined attempt of the r pass: its grid nD + nP + npad (fcd_ctx_stat "pipe_grid") ...
    int64_t pipe_capacity;         // ... and the workgroups resident at once for it, pipe_occ * num_cu ("pipe_capacity")
    int r_form_last;               // form of the last blocked r pass: 1 step-per-launch, 2 pipelined, 3 one-launch with counters,
                                   // 4 sparse (knob r_sure) (fcd_ctx_stat)
    long long n_pack;              // packing launches of the r pass so far (fcd_ctx_stat "pack_launches")
    long long n_pack_tally;        // ... of them that carried the f half of the tally (fcd_ctx_stat "tally_f_in_pack")
    long long n_r_tally;           // pipelined r pass launches that carried it (fcd_ctx_stat "tally_f_in_r")
    long long n_f_tally;           // f passes whose run kernel counted it (fcd_ctx_stat "tally_f_in_f")
    long long n_frec_pass;         // f passes that read prebuilt pair records (fcd_ctx_stat "f_rec_passes")
    long long n_frec_build;        // launches of the kernel that builds them (fcd_ctx_stat "f_rec_builds")
    long long n_fsure_pass;        // f passes that ran the kernel with the decided-tile path (fcd_ctx_stat "f_sure_passes")
    long long n_frun_pass;         // ... of them in the run form, gibbs_f_run_kernel (fcd_ctx_stat "f_run_passes")
    long long n_rsure_pass;        // r passes in the sparse form (fcd_ctx_stat "r_sure_passes")
    long long n_rsure_build;       // launches of the kernel that builds its site bounds (fcd_ctx_stat "r_sure_builds")
    volatile fcd_hint_words *hint;     // pinned host words of the two hint builds
    void *log_tab;     // K_lik tables (fcd_fastmath.h): 64 x 2^(-j/64), 512 x {1/m_i, log m_i} (device, 8.5 KiB)
    volatile unsigned *dev_err;   // pinned host word: error word of the one-launch r pass (FCD_DEV_ERR_*), polled by its kernels
    void *acc;         // FCD_ACC_BYTES: 8 x uint64, zero between launches: the tally's pooled sums [0..3] and its ticket [4]
    void *f_slots;     // FCD_F_SLOTS 64-byte lines of 8 x uint64, zero between sweeps: the pooled f counts of a run kernel that counts
                       // ([0] zeros, [1] ones, [2] twos of a line), spread so that its workgroups do not queue on acc's line;
                       // folded into acc[1..3] by the r pass behind it (fcd_f_slots_fold)
    void *nan_slots;   // FCD_NAN_SLOTS 128-byte lines of 16 x uint64, zero between launches: K_lik's per-block NaN counts
                       // ([0] b, [1] bt of a line), spread so that its blocks do not queue on one address
    void *comm;        // ncclComm_t of the context (fcd_comm_init), or nullptr: fcd_gibbs_run pools its M-step counts over it
    int comm_world, comm_rank;
    void *pool_counts; // 8 x int64 (device): the counts vector the all-reduce works on in place
    fcd_dev_words *words;          // device (see the struct)
    fcd_dev_buf corr_tickets = {nullptr, 0, 0, true, false};   // K_corr: one ticket per subject, zero between launches (the last taker resets it)
    fcd_dev_buf fsq = {nullptr, 0, 0, false, true};    // square copy of the f state [w][n][m][lane] the sweep loop keeps between its f and r pass
    fcd_dev_buf frec = {nullptr, 0, 0, false, true};   // pair records and edge constants of the pair-tile f pass (fcd_sweep_plan::frec_bytes), valid
                                                       // inside ONE sweep-loop call: it makes them from that call's lMf before the first pass that reads them
    // per-subject constants of the measurement-noise tables (fcd_lik_sessions.hip), valid inside ONE call: six doubles per
    // control and per patient session, made by that call's first launch
    fcd_dev_buf noise_rec = {nullptr, 0, (size_t)64 << 10, false, true};
    fcd_sweep_acc sweep_acc[FCD_ACC_N];
    fcd_dev_buf count_ws = {nullptr, 0, 0, false, true};       // per-chain counts of one tally, (U + Nreg) rows of GW*64 uint16 (fcd_count_ws_reserve)
    // region sets (fcd_region_sets_set): J + 1 offsets, then the members (CSR, int32, device; owned), checked on the host
    void *rs_dev;
    int64_t rs_J, rs_smax, rs_max_member = -1; // number of sets (0: none), largest set, largest member
    // patient groups and contrasts (fcd_patient_groups_set): one device buffer (owned; layout in fcd_patient_groups.hip) of the
    // CSR, the contrasts, a bit mask over u per group and the contrasts' bin offsets, checked on the host
    void *pg_dev;
    int64_t pg_J, pg_P, pg_umax, pg_max_member = -1;   // groups (0: none), contrasts, largest group, largest member
    int64_t pg_total, pg_bins_max;                     // members in all groups; joint bins of the largest contrast
    int pg_with_rs;                                    // 1: the context's region sets are rows after the regions
    // patient traits (fcd_patient_traits_set): one device buffer (owned) of the words 2 score + known (Q, U) and the numbers
    // of known patients (Q), checked on the host
    void *pt_dev;
    int64_t pt_Q, pt_U, pt_umax;                       // traits (0: none), the patients they were set for, largest n_q
    int pt_with_rs;                                    // 1: the context's region sets are rows after the regions
    // optional per-kernel timing with HIP events on the launch stream (fcd_prof_enable / fcd_prof_collect)
    int prof_on;
    hipEvent_t *prof_ev[FCD_PROF_SLOTS];   // pairs (begin, end)
    int prof_n[FCD_PROF_SLOTS];            // pairs recorded
    int prof_cap[FCD_PROF_SLOTS];
    char msg[256];
};

#define FCD_HIP_TRY(expr)                       \
    do {                                        \
        hipError_t e__ = (expr);                \
        if (e__ != hipSuccess) return (int)e__; \
    } while (0)

#define FCD_LAUNCH_CHECK()                      \
    do {                                        \
        hipError_t e__ = hipGetLastError();     \
        if (e__ != hipSuccess) return (int)e__; \
    } while (0)

static inline int fcd_fail(fcd_ctx *ctx, int code, const char *fmt, long long a = 0, long long b = 0) {
    if (ctx) snprintf(ctx->msg, sizeof(ctx->msg), fmt, a, b);
    return code;
}
// the same for a message "<who>: <text>", text = fmt with its numbers (`who` is a name, not a format)
static inline int fcd_fail_who(fcd_ctx *ctx, int code, const char *who, const char *fmt, long long a = 0, long long b = 0) {
    if (ctx) {
        char tail[192];
        snprintf(tail, sizeof(tail), fmt, a, b);
        snprintf(ctx->msg, sizeof(ctx->msg), "%s: %s", who, tail);
    }
    return code;
}
// The alignment contract of include/fcdiff_hip.h: a device pointer whose kernels read or write it as 16-byte vectors must be
// 16-byte aligned (DESIGN.md has the table of them).  Checked on the host before any launch; a null pointer passes (an
// entry point refuses or accepts a null argument by its own rules).
static inline int fcd_fail_align16(fcd_ctx *ctx, const char *who, const char *name) {
    if (ctx) snprintf(ctx->msg, sizeof(ctx->msg), "%s: argument %s must be 16-byte aligned", who, name);
    return FCD_ERR_ARG;
}
#define FCD_ALIGN16(ctx, who, name, ptr)                                                         \
    do {                                                                                         \
        if ((uintptr_t)(const void *)(ptr) & 15u) return fcd_fail_align16((ctx), (who), (name)); \
    } while (0)

// What the fcd_gibbs_set_*_accumulator entry points share: all buffers null detaches, else the checks and the store.  The
// message texts are the caller's (fcd_fail formats numbers only); msg_limit is non-null where the shape is past a limit of
// the caller's own kernels.
static inline int fcd_sweep_acc_set(fcd_ctx *ctx, int slot, uint32_t *b0, uint32_t *b1, int64_t Nreg, int64_t U, int64_t every,
                                    const char *msg_together, const char *msg_shape, const char *msg_limit,
                                    const char *msg_every) {
    if (!ctx) return FCD_ERR_ARG;
    if (!b0 && !b1) {
        ctx->sweep_acc[slot] = fcd_sweep_acc{{nullptr, nullptr}, 0, 0, 1};
        return FCD_OK;
    }
    if (!b0 || !b1) return fcd_fail(ctx, FCD_ERR_ARG, msg_together);
    if (Nreg < 2 || U < 1) return fcd_fail(ctx, FCD_ERR_SHAPE, msg_shape, Nreg, U);
    if (msg_limit) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, msg_limit, Nreg, U);
    if (every < 1) return fcd_fail(ctx, FCD_ERR_ARG, msg_every, every);
    ctx->sweep_acc[slot] = fcd_sweep_acc{{b0, b1}, Nreg, U, every};
    return FCD_OK;
}

// A kernel whose table addresses assume that its dynamic LDS array starts at address 0 must declare no static LDS:
// asked of the runtime once per kernel (*done)
static inline int fcd_static_lds_check(fcd_ctx *ctx, const void *fn, int *done) {
    if (*done) return FCD_OK;
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, fn);
    if (e != hipSuccess) return (int)e;
    if (fa.sharedSizeBytes != 0) {
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "kernel carries %lld bytes of static LDS: its table addresses assume none",
                        (long long)fa.sharedSizeBytes);
    }
    *done = 1;
    return FCD_OK;
}

int fcd_comm_allreduce_counts(fcd_ctx *ctx, long long *counts, hipStream_t stream);     // fcd_comm.hip: no-op without a communicator
// grow a context-owned block to at least this many bytes (no HIP call where it is large enough); a failed growth leaves it empty
int fcd_buf_reserve(fcd_ctx *ctx, fcd_dev_buf &b, size_t bytes);
static inline int fcd_ws_reserve(fcd_ctx *ctx, size_t bytes) { return fcd_buf_reserve(ctx, ctx->ws, bytes); }
// fcd_corr_edges for a caller inside the library (fcd_corr_partial): its scratch starts ws_off bytes into the context's
// workspace (the caller's own lies in front; `out` may point there once the caller has reserved ws_off +
// fcd_corr_edges_ws_bytes), and the subject kernel slices the time axis as a call of S_slices subjects would -- a caller that
// walks its subjects in chunks passes the whole call's S, so that the chunking changes no bit.  fcd_corr_edges is (.., 0, S, ..).
int fcd_corr_edges_at(fcd_ctx *ctx, const double *ts, int64_t S, int64_t Nreg, int64_t T, int fisher_z, double *out, size_t ws_off,
                      int64_t S_slices, hipStream_t stream);
size_t fcd_corr_edges_ws_bytes(const fcd_ctx *ctx, int64_t S, int64_t Nreg, int64_t T, int64_t S_slices);
// The front half of fcd_corr_partial for a caller inside the library (fcd_corr_partial itself, fcd_tangent_*): one chunk of Sc
// subjects from time series to the dense shrunk correlation matrices.  A (Sc, PL, PL), PL = 16 ceil(Nreg / 16): R_alpha on the
// live block, identity rows for dead and padding regions and for every row of a subject whose status is set; alpha and
// info (p_live, status 0 / 2 / 3) at s0 + s of the call's arrays; the live flags (Sc, PL) int32 at w.o_live.  The plan lays
// the scratch out from `base` bytes into the context's workspace (the caller reserves w.end + its own + edges_off's
// fcd_corr_edges_ws_bytes); A may lie anywhere on the device: w.o_A is the slot the plan keeps for it, none with
// with_A = false.  S_call as fcd_corr_edges_at's S_slices: the chunking changes no bit.
struct fcd_shrunk_ws {
    size_t o_redge, o_A, o_live, o_rowF, o_F, o_mean, o_isd, o_q, end;
    int PL, RT, NBT;
};
void fcd_corr_shrunk_plan(int64_t SC, int64_t Nreg, int64_t T, size_t base, fcd_shrunk_ws &w, bool with_A = true);
int fcd_corr_shrunk_at(fcd_ctx *ctx, const double *x, int64_t Sc, int64_t Nreg, int64_t T, const int32_t *n_frames, int64_t s0,
                       int64_t S_call, int shrink_mode, double shrink_value, const fcd_shrunk_ws &w, size_t edges_off, double *A,
                       double *alpha, int32_t *info, hipStream_t stream);
// raise a kernel's dynamic-LDS limit if this size was not set before (no HIP call otherwise)
static inline int fcd_lds_attr(fcd_ctx *ctx, int slot, const void *fn, size_t shmem) {
    if (shmem <= 64 * 1024 || shmem <= ctx->lds_attr[slot]) return FCD_OK;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return (int)e;
    ctx->lds_attr[slot] = shmem;
    return FCD_OK;
}
// The f half of the tally (pooled counts of f, marginal counters of the edges): it needs nothing of the r pass, so the r
// pass's packing launch can carry it in extra workgroups of its own instead of the tally launch after the pass -- and the f
// pass's run kernel can leave the same sums as it stores the draws, without reading the state back (cnt_f: atomic adds; the
// pooled sums through the slot lines of fcd_f_slots_fold, not into acc's one line).
struct fcd_tally_f {
    const uint8_t *f_state;
    int64_t C, G;
    int GW;
    unsigned long long *acc;           // nullable: context-owned sums, [1..3] = number of f == 0, 1, 2
    uint32_t *cnt_f;                   // nullable
};
// The pipelined r pass carries it too, in its in-order workgroups (16 waves each, nD of them), which can do nothing before
// the first panel step has published its values.  Only where that wait covers the count: a wave walks
// R = ceil(C / (64 nD)) * ceil(GW / 16) rounds of four edges x 16 chain words, and the pass carries the f half where
// R <= R_TALLY_MAX_ROUNDS (cfg3: R = 4; few patients mean few in-order workgroups and many rounds, which would sit on the
// pass's serial path).  Measured at Nreg 200, 1024 chains (profiles/tally_in_r_pass_cfg3.txt): per launch that carries it the
// pass grows by 0.7 us at R = 4 and 0.4-1.6 us at R = 5 -- inside what repeated runs differ by -- and by 7-8 us at R = 6 and 7.
constexpr int R_TALLY_MAX_ROUNDS = 5;
// one launch of the (f_c, mixture case) count kernel of fcd_post.hip: acc (C, U, 3, 3) = (accumulate ? acc : 0) + counts of
// this state; T = uint32_t or double
struct fcd_geo;
template <typename T>
int fcd_pair_tally_launch(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                          const fcd_geo &g, T *acc, bool accumulate, hipStream_t s);
// the anomalous-region count kernels of fcd_count.hip (two launches): both histograms += the counts of this state; the
// scratch they need is grown by fcd_count_ws_reserve (fcd_gibbs_run: before its sweep loop, through its table of the slots,
// which is why the four *_ws_reserve take the same arguments)
int fcd_count_ws_reserve(fcd_ctx *ctx, int64_t Nreg, int64_t U, int64_t G);
int fcd_count_tally_launch(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, const fcd_geo &g,
                           uint32_t *hist_patient, uint32_t *hist_region, hipStream_t s);
// the co-anomaly kernel of fcd_coanomaly.hip (one launch, no scratch): both pair matrices += the counts of this state
int fcd_coanomaly_tally_launch(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, const fcd_geo &g,
                               uint32_t *region_pairs, uint32_t *patient_pairs, hipStream_t s);
// the region-set kernels of fcd_region_sets.hip (two launches): both histograms += the counts of this state over the
// context's sets; their scratch is the count tally's, grown by fcd_region_set_ws_reserve (fcd_gibbs_run: before its loop)
int fcd_region_set_ws_reserve(fcd_ctx *ctx, int64_t Nreg, int64_t U, int64_t G);
int fcd_region_set_tally_launch(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, const fcd_geo &g,
                                uint32_t *hist_set, uint32_t *hist_prev, hipStream_t s);
// the patient-group kernels of fcd_patient_groups.hip (two launches): both histograms += the counts of this state over the
// context's groups and contrasts; same scratch, grown by fcd_patient_group_ws_reserve (fcd_gibbs_run: before its loop)
int fcd_patient_group_ws_reserve(fcd_ctx *ctx, int64_t Nreg, int64_t U, int64_t G);
int fcd_patient_group_tally_launch(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, const fcd_geo &g,
                                   uint32_t *hist_group, uint32_t *hist_joint, hipStream_t s);
// the patient-trait kernels of fcd_patient_traits.hip (two launches): histogram and sums += the rank-sum statistics of this
// state over the context's traits; same scratch, grown by fcd_patient_trait_ws_reserve (fcd_gibbs_run: before its loop)
int fcd_patient_trait_ws_reserve(fcd_ctx *ctx, int64_t Nreg, int64_t U, int64_t G);
int fcd_patient_trait_tally_launch(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, const fcd_geo &g,
                                   uint32_t *trait_hist, int64_t *trait_sum, hipStream_t s);
// bracket ONE kernel launch with events when profiling is on (no-ops otherwise)
void fcd_prof_begin(fcd_ctx *ctx, int slot, hipStream_t s);
void fcd_prof_end(fcd_ctx *ctx, int slot, hipStream_t s);

// hyper block offsets
#define FCD_H_LNGAMMA 0
#define FCD_H_LNPI0 3
#define FCD_H_LNPI1 4

// RNG kinds (4th counter word)
#define FCD_KIND_INIT_F 0u
#define FCD_KIND_INIT_R 1u
#define FCD_KIND_F 2u
#define FCD_KIND_R 3u

// ---------------------------------------------------------------------------------------------
// edge <-> region-pair maps, fcdiff/util.py:40-84.  c = n(n-1)/2 + m, n > m.
// ---------------------------------------------------------------------------------------------
__host__ __device__ static inline int64_t fcd_tri(int64_t n) { return n * (n - 1) / 2; }

// Inverse with an integer correction step (the reference's float sqrt formula, util.py:82, is only
// trusted near perfect squares up to the sizes it was written for).
__host__ __device__ static inline void fcd_edge_to_pair(int64_t c, int &n, int &m) {
    int64_t nn = (int64_t)((sqrt(8.0 * (double)c + 1.0) - 1.0) * 0.5) + 1;
    while (fcd_tri(nn) > c) --nn;
    while (fcd_tri(nn + 1) <= c) ++nn;
    n = (int)nn;
    m = (int)(c - fcd_tri(nn));
}

// Edge id the region update uses for the ORDERED pair (n, m), m != n.
__host__ __device__ static inline int64_t fcd_pair_to_edge(int n, int m, int mode) {
    if (mode == FCD_EDGE_REFERENCE || n > m) return fcd_tri(n) + m;  // fit.py:186 / util.py:60
    return fcd_tri(m) + n;
}

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 (Random123 constants).  counter = (idx, chain, sweep, kind), key = seed.
// ---------------------------------------------------------------------------------------------
struct fcd_u4 {
    uint32_t x, y, z, w;
};

__host__ __device__ static inline fcd_u4 fcd_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                    uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return fcd_u4{c0, c1, c2, c3};
}

// 53 high bits of (hi:lo) as a double in [0, 1).
__host__ __device__ static inline double fcd_u53(uint32_t hi, uint32_t lo) {
    uint64_t w = ((uint64_t)hi << 32) | lo;
    return (double)(w >> 11) * (1.0 / 9007199254740992.0);
}

// One 32-bit word as a double in [0, 1): what the 3-way f draws of the sweeps use (four edges per counter block).
__host__ __device__ static inline double fcd_u32(uint32_t w) { return (double)w * (1.0 / 4294967296.0); }
__host__ __device__ static inline uint32_t fcd_word(const fcd_u4 &x, int i) { return i == 0 ? x.x : i == 1 ? x.y : i == 2 ? x.z : x.w; }

__host__ __device__ static inline double fcd_site_uniform(uint64_t seed, uint32_t idx, uint32_t chain,
                                                          uint32_t sweep, uint32_t kind, int half) {
    fcd_u4 x = fcd_philox(idx, chain, sweep, kind, (uint32_t)seed, (uint32_t)(seed >> 32));
    return half ? fcd_u53(x.z, x.w) : fcd_u53(x.x, x.y);
}

// ---------------------------------------------------------------------------------------------
// draws: identical formulas in oracle/fcdiff_oracle.py (draw_f, draw_r) and oracle/fcdiff_oracle.c
// ---------------------------------------------------------------------------------------------
__device__ static inline int fcd_draw_f(double a0, double a1, double a2, double x) {
    double mx = fmax(a0, fmax(a1, a2));
    double e0 = exp(a0 - mx), e1 = exp(a1 - mx), e2 = exp(a2 - mx);
    double t = x * ((e0 + e1) + e2);
    return (t < e0) ? 0 : ((t < e0 + e1) ? 1 : 2);
}

// The same draw from three hardware fp32 exponentials (~20 instructions instead of ~150), for log-odds b1, b2 against type 0
// that are themselves only known to within +-delta (fp32 accumulation of the f pass; 0 for fp64 sums).  *amb is set when the
// outcome could be another one in exact arithmetic: the caller then repeats the draw with fcd_draw_f on fp64 sums, so the
// outcome is always fcd_draw_f's.  After the shift by the largest exponent ONE weight is exactly 1; the other two carry a
// relative uncertainty eta = e^(2 delta) - 1 (both b's off in opposite directions) + 2e-5 (fp32 exp: argument rounding
// times |argument| <= 87, then 1 ulp), so x * sum and either boundary move by at most eta * (sum - 1) each -- an
// uncertainty RELATIVE TO THE WEIGHT OFF THE MODE, not to the sum: a conditional that is all but one-hot (the usual case)
// never repeats on account of it.  `floor_rel` * sum covers the fp32 roundings of x, the sum and the product (default
// FCD_DRAW_F_MARGIN; the test hook f_tol raises it: 1e30 sends every draw down the exact path).  NaN-safe: a NaN or
// infinite sum or bound is ambiguous.
#define FCD_DRAW_F_MARGIN 1e-6f
__host__ __device__ static inline float fcd_draw_f_eta(float delta) { return expm1f(2.0f * delta) * 1.001f + 2e-5f; }
__device__ static inline int fcd_draw_f_fast(double b1, double b2, double x, float eta, float floor_rel, bool *amb) {
    const double mx = fmax(0.0, fmax(b1, b2));
    const float e0 = __expf((float)(0.0 - mx)), e1 = __expf((float)(b1 - mx)), e2 = __expf((float)(b2 - mx));
    const float s = (e0 + e1) + e2;
    const float t = (float)x * s;
    const float m = 2.0f * eta * (s - 1.0f) + floor_rel * s;
    *amb = !(fabsf(t - e0) >= m && fabsf(t - (e0 + e1)) >= m);
    return (t < e0) ? 0 : ((t < e0 + e1) ? 1 : 2);
}
// The draw entirely in fp32 (the pair forms of the f pass: their sums are fp32 already): bf1, bf2 = log-odds against type 0
// known to within +-delta, eta = fcd_draw_f_eta(delta), xf = the uniform rounded to fp32 (covered by floor_rel).  Same rule,
// same outcomes.
__device__ static inline int fcd_draw_f_fast32(float bf1, float bf2, float xf, float eta, float floor_rel, bool *amb) {
    const float mx = fmaxf(0.f, fmaxf(bf1, bf2));
    const float e0 = __expf(0.f - mx), e1 = __expf(bf1 - mx), e2 = __expf(bf2 - mx);
    const float s = (e0 + e1) + e2;
    const float t = xf * s;
    const float m = 2.0f * eta * (s - 1.0f) + floor_rel * s;
    *amb = !(fabsf(t - e0) >= m && fabsf(t - (e0 + e1)) >= m);
    return (t < e0) ? 0 : ((t < e0 + e1) ? 1 : 2);
}
// The draw without an exponential, where it is certain: if the largest of (0, b1, b2) leads the second by more than 15 + eta
// (eta >= twice the sums' error bound), the two other weights together are below 2 e^-15 = 6.1e-7 of the largest, and any x in
// [1e-6, 1 - 1e-6] falls into the largest one's interval of the inverse CDF whatever the order of the three: k = argmax,
// exactly what fcd_draw_f returns.  Returns false where that cannot be said (the caller then takes fcd_draw_f_fast32).
// On well separated data nearly every draw is of this kind; on weak data the test costs a dozen instructions.
__device__ static inline bool fcd_draw_f_sure(float bf1, float bf2, float xf, float eta, int *k) {
    const float mx = fmaxf(0.f, fmaxf(bf1, bf2)), mn = fminf(0.f, fminf(bf1, bf2));
    const float mid = ((bf1 + bf2) - mx) - mn;                        // (the middle one of 0, b1, b2, to within rounding: covered by the 1e-2)
    *k = (bf2 >= mx) ? 2 : ((bf1 >= mx) ? 1 : 0);
    return (mx - mid) - eta > 15.01f && xf > 1e-6f && xf < 0.999999f;
}
// absolute error bound of an fp32 sum of n terms, each first rounded to fp32, given B >= sum of |terms|: the n conversions
// cost at most 2^-24 B together, each of the n - 1 additions at most 2^-24 times a partial sum of magnitude <= B
__host__ __device__ static inline float fcd_f32_sum_err(int n_terms, float B) { return (float)(n_terms + 1) * 5.97e-8f * 1.01f * B; }
// ... and of  (float)c + that sum  for an offset |c| <= cm: the offset's conversion and one more addition
__host__ __device__ static inline float fcd_f32_offset_err(float cm, float B) { return 2.0f * 5.97e-8f * 1.01f * (cm + B); }

// r = 1 with probability sigmoid(s1 - s0):  x < 1/(1+exp(s0-s1))  <=>  logit(x) < s1 - s0.
// The threshold depends on the random number only, so it is computed off the region-to-region chain.
__device__ static inline double fcd_logit(double x) { return log(x / (1.0 - x)); }
__device__ static inline int fcd_draw_r(double s0, double s1, double x) { return fcd_logit(x) < (s1 - s0) ? 1 : 0; }
// logit(x) to within FCD_LOGIT_FAST_ERR (absolute) from two hardware fp32 logarithms (8 instructions instead of a
// double-precision division and logarithm).  A draw decided with it is re-decided with fcd_logit whenever the
// compared quantity lies within the tolerance, so the outcome is always that of fcd_logit.
#define FCD_LOGIT_FAST_ERR 2e-5
__device__ static inline double fcd_logit_fast(double x) {
    const float a = __log2f((float)x), b = __log2f((float)(1.0 - x));   // x = 0 -> -inf, like fcd_logit
    return (double)((a - b) * 0.69314718f);
}

// ---------------------------------------------------------------------------------------------
// wave64 helpers
// ---------------------------------------------------------------------------------------------
__device__ static inline double fcd_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// per-lane select driven by a wave-uniform 64-bit mask held in an SGPR pair:
// lane i gets (mask bit i) ? b : a.  One v_cndmask_b32, no per-lane shift.
__device__ static inline uint32_t fcd_sel_mask(uint32_t a, uint32_t b, uint64_t mask) {
    uint32_t out;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(out) : "v"(a), "v"(b), "s"(mask));
    return out;
}

// mask of the chains of word w that exist (the last word of G chains may be partial)
__host__ __device__ static inline uint64_t fcd_active_mask(int w, int64_t G) {
    const int64_t rem = G - (int64_t)w * 64;
    return rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
}

#ifdef __HIPCC__
constexpr int R_NB = 16;   // regions per diagonal block of the blocked r pass (even: both halves of a Philox block stay inside)
// 8 two-bit fields of x -> the low two bits of 8 bytes (x: fields 0-3, y: fields 4-7)
__device__ __forceinline__ uint2 spread2(uint32_t x16) {
    uint32_t lo = x16 & 0xFFu, hi = (x16 >> 8) & 0xFFu;
    lo = (lo | (lo << 12)) & 0x000F000Fu;
    hi = (hi | (hi << 12)) & 0x000F000Fu;
    lo = (lo | (lo << 6)) & 0x03030303u;
    hi = (hi | (hi << 6)) & 0x03030303u;
    return make_uint2(lo, hi);
}
// the r word of (w, u, b) the blocked r pass reads (r_S, fcd_gibbs_r.hip): bit j = r_{16 b + j, u} of this lane's chain,
// one byte per pair of regions
// (the whole wave, (w, u, b) wave-uniform: lane l loads the word of region 16 b + l % 16 -- ONE memory instruction instead of 16 --
// and every lane takes its bit of each word from the lane that holds it)
__device__ __forceinline__ uint64_t fcd_lane_word(uint64_t v, int j) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint2 fcd_r_pair_bytes(const uint64_t *__restrict__ r_bits, int Nreg, int U, int w, int u, int b,
                                                  int lane) {
    const int ml = b * R_NB + (lane & (R_NB - 1));
    const uint64_t mine = r_bits[((int64_t)w * Nreg + (ml < Nreg ? ml : Nreg - 1)) * U + u];    // clamped: no branch around the load
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < R_NB; ++j) {
        const int m = b * R_NB + j;
        v |= (m < Nreg ? (uint32_t)((fcd_lane_word(mine, j) >> lane) & 1ull) : 0u) << j;
    }
    return spread2(v);
}

// DPP move of a 32-bit word inside the rows of 16 lanes (every lane reads a lane that exists: no bound control needed)
template <int CTRL>
__device__ __forceinline__ uint32_t fcd_dpp_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
// Four per-lane values -> their four sums over the wave, in one tree: lane l ends with the sum of p[l & 3].  The first two
// steps halve the number of values instead of doubling the number of copies (a lane keeps the value of its own parity and
// hands over the other), so the tree is 3 + 2 DPP moves and two cross-row exchanges for FOUR sums, against 6 exchanges
// for each.  No sum may exceed 32 bits -- the caller packs two 16-bit counts in a word.
__device__ __forceinline__ uint32_t fcd_wave_sum4(const uint32_t (&p)[4], int lane) {
    const bool b0 = lane & 1, b1 = lane & 2;
    const uint32_t x01 = (b0 ? p[1] : p[0]) + fcd_dpp_u32<0xB1>(b0 ? p[0] : p[1]);      // quad_perm [1,0,3,2]
    const uint32_t x23 = (b0 ? p[3] : p[2]) + fcd_dpp_u32<0xB1>(b0 ? p[2] : p[3]);
    uint32_t y = (b1 ? x23 : x01) + fcd_dpp_u32<0x4E>(b1 ? x01 : x23);                  // quad_perm [2,3,0,1]: p[l & 3] over the quad
    y += fcd_dpp_u32<0x124>(y);             // row_ror:4 and row_ror:8 keep l & 3: the four quads of the row
    y += fcd_dpp_u32<0x128>(y);
    y += __shfl_xor(y, 16, 64);             // the four rows
    y += __shfl_xor(y, 32, 64);
    return y;
}

// The f half of the tally for workgroup lin of nblk (WAVES waves each): f_state is read once, 16 bytes per lane -- a wave
// covers the 16 chain words x 64 chains of an edge with one load instruction; four edges per round, their loads issued
// together (the pass is a few memory round trips long: what counts is the number of bytes in flight).  red: LDS,
// [WAVES][3].  Integer sums: any order gives the same totals.
// The counters: wave (lin, wave) is the only one of the launch that meets edges c0 .. c0 + 3 (every caller numbers its
// workgroups lin = 0 .. nblk - 1 once each, and the groups of chain words of an edge are a loop of the same wave), and
// launches that count follow each other in one stream -- so the twelve words cnt_f[3 c0 .. 3 c0 + 11] are read, added to
// and stored by lanes 0 .. 11, the old values asked for together with the f state.  (They were four atomics per edge from
// lane 0.)
// The pooled f counts of a run kernel that counts (fcd_gibbs.hip, gibbs_f_run_kernel): every workgroup adds its three sums to
// one of FCD_F_SLOTS lines instead of acc's one -- same-address atomics serialise at the memory side, about 80 per us, and 4200
// of them at cfg3 made the kernel 26 us longer (profiles/f_run_counts_cfg3.txt).  ONE wave of a later launch in the stream,
// before the tally, takes the lines (and leaves them zero) and adds the totals to acc[1..3]: three atomics in all.
__device__ __forceinline__ void fcd_f_slots_fold(unsigned long long *slots, unsigned long long *acc, int lane) {
    static_assert(FCD_F_SLOTS == 64, "one line per lane");
    unsigned long long v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = atomicExch(&slots[lane * 8 + k], 0ull);     // (read at the memory side and reset)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if (lane == 0 && v[k]) (void)__hip_atomic_fetch_add(acc + 1 + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int WAVES>
__device__ __forceinline__ void fcd_tally_f_block(const fcd_tally_f &a, int lin, int nblk, unsigned long long (*red)[3]) {
    const uint8_t *__restrict__ f_state = a.f_state;
    uint32_t *cnt_f = a.cnt_f;
    const int64_t C = a.C, G = a.G;
    const int GW = a.GW;
    // (the wave's number as a scalar: the walk over the edges, its bounds and the totals then live in scalar registers)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sub = lane & 3, wrow = lane >> 2;          // 16-byte piece of the 64-byte row, chain word within a group of 16
    unsigned long long tot1 = 0, tot2 = 0, n_edges = 0;  // (wave-uniform)
    const int own_e = ((lane * 11) >> 5) & 3, own_j = lane - 3 * own_e;      // lane / 3, lane % 3 for the twelve lanes that store
    constexpr int TE = 4;
    for (int64_t c0 = ((int64_t)lin * WAVES + wave) * TE; c0 < C; c0 += (int64_t)nblk * WAVES * TE) {
        const int ne = (int)(C - c0 < TE ? C - c0 : TE);
        const bool owner = cnt_f && lane < 3 * ne;       // lane l: counter l % 3 of edge c0 + l / 3
        uint32_t old = 0;
        if (owner) old = cnt_f[c0 * 3 + lane];
        uint32_t s1 = 0, s2 = 0;                         // lane l: ones and twos of edge c0 + (l & 3), over the groups so far
        for (int wg = 0; wg < GW; wg += 16) {
            const int w = wg + wrow;
            uint4 vv[TE];
#pragma unroll
            for (int t = 0; t < TE; ++t) {
                const int64_t c = (c0 + t < C) ? c0 + t : C - 1;
                vv[t] = *reinterpret_cast<const uint4 *>(f_state + ((int64_t)(w < GW ? w : 0) * C + c) * 64 + sub * 16);
            }
            const uint32_t act = (w < GW) ? (uint32_t)(fcd_active_mask(w, G) >> (sub * 16)) & 0xFFFFu : 0u;
            uint32_t p[TE];                              // ones | twos << 16: a group's sum per edge is at most 1024
#pragma unroll
            for (int t = 0; t < TE; ++t) {
                uint4 v = vv[t];
                if (act != 0xFFFFu) {   // partial (or absent) chain word: drop the bytes of chains that do not exist
                    v.x &= (((act & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu;
                    v.y &= ((((act >> 4) & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu;
                    v.z &= ((((act >> 8) & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu;
                    v.w &= ((((act >> 12) & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu;
                }
                const uint32_t ones = __popc(v.x & 0x01010101u) + __popc(v.y & 0x01010101u) + __popc(v.z & 0x01010101u) +
                                      __popc(v.w & 0x01010101u);
                const uint32_t twos = __popc(v.x & 0x02020202u) + __popc(v.y & 0x02020202u) + __popc(v.z & 0x02020202u) +
                                      __popc(v.w & 0x02020202u);
                p[t] = ones | (twos << 16);
            }
            const uint32_t s = fcd_wave_sum4(p, lane);
            s1 += s & 0xFFFFu;
            s2 += s >> 16;
        }
        // the pooled totals as wave-uniform sums (lanes 0 .. 3 hold the four edges); every owner takes its edge's pair
#pragma unroll
        for (int t = 0; t < TE; ++t) {
            if (t < ne) {      // (an edge past the last was read as a copy of the last)
                tot1 += (uint32_t)__builtin_amdgcn_readlane((int)s1, t);
                tot2 += (uint32_t)__builtin_amdgcn_readlane((int)s2, t);
            }
        }
        const uint32_t ones = __shfl(s1, own_e, 64), twos = __shfl(s2, own_e, 64);
        const uint32_t add = own_j == 0 ? (uint32_t)G - ones - twos : (own_j == 1 ? ones : twos);
        n_edges += (unsigned long long)ne;
        if (owner) cnt_f[c0 * 3 + lane] = old + add;
    }
    if (!a.acc) return;
    // one set of atomics per workgroup (same-address atomics serialise): wave sums -> LDS -> threads 0..2
    if (lane == 0) {
        red[wave][0] = n_edges * (unsigned long long)G - tot1 - tot2;
        red[wave][1] = tot1;
        red[wave][2] = tot2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long t = 0;
        for (int q = 0; q < WAVES; ++q) t += red[q][threadIdx.x];
        if (t) {
            // with the old value asked for, the add has been performed at the memory side once it returns (every access
            // to acc[] is a device-scope atomic): whoever takes a ticket after this workgroup's barrier finds it there
            const unsigned long long old = atomicAdd(&a.acc[1 + threadIdx.x], t);
            asm volatile("" ::"v"(old));
        }
    }
    __syncthreads();
}
#endif

// ---------------------------------------------------------------------------------------------
// host: shape checks shared by the sampler entry points
// ---------------------------------------------------------------------------------------------
struct fcd_geo {
    int64_t C;
    int GW;
};

static inline int fcd_geo_check(fcd_ctx *ctx, int64_t Nreg, int64_t U, int64_t G, int64_t chain0, fcd_geo &g) {
    if (!ctx) return FCD_ERR_ARG;
    if (Nreg < 2 || U < 1 || G < 1)
        return fcd_fail(ctx, FCD_ERR_SHAPE, "need Nreg >= 2, U >= 1, G >= 1 (Nreg=%lld, U=%lld)", Nreg, U);
    if (Nreg > 46340 || U > (1 << 20) || G > (1ll << 31) || chain0 < 0 || chain0 + G > (1ll << 32))
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "shape out of range (Nreg=%lld, G=%lld)", Nreg, G);
    g.C = fcd_tri(Nreg);
    g.GW = (int)((G + 63) / 64);
    if (g.GW > 65535) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "G=%lld exceeds 65535 chain words per launch", G);
    if ((Nreg + 1) / 2 * U > (1ll << 32) || (g.C + 1) / 2 > (1ll << 32))
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "site index exceeds the 32-bit counter word");
    return FCD_OK;
}

// ---------------------------------------------------------------------------------------------
// host: the plan of a sweep at one shape (fcd_sweep_plan_for, fcd_gibbs_r.hip): the ONE place that decides which form each
// pass runs and where its scratch lies.  fcd_ctx_reserve, both passes and the sweep loop read it.  It depends on the shape
// and the knobs; a call adds whether lMf (the f forms) and lMd (the blocked r pass) are there, and its edge ids.
// ---------------------------------------------------------------------------------------------
enum { FCD_F_GENERIC = 0, FCD_F_PAIR = 1, FCD_F_PAIRX = 2, FCD_F_DIFF = 3 };   // f pass forms (knob f_form: 2, 3)
constexpr int FP_EC = 8;     // edges per tile of the U <= 64 pair kernel
constexpr int FT_W = FP_EC / 2;      // ... columns of a pair-aligned tile (two rows of the triangle)
__host__ __device__ static inline int64_t fpt_tiles(int64_t i) {       // pair-aligned tiles of the row pairs before i
    const int64_t j = i >> 1;
    return (i & 1) ? (j + 1) * (j + 1) : j * (j + 1);
}
// Block-wide runs of pair-aligned tiles (fcd_gibbs.hip, gibbs_f_run_kernel): run t is the tiles of one row pair (n0, n0 + 1)
// whose columns lie in one block of FR_W = 16 regions (R_NB), [mb, mb + FR_W): up to four tiles, 32 edges, edge e = (row e / FR_W,
// column e % FR_W), present where e % FR_W < cnt of its row, id cr + e % FR_W.  Row pair i has floor(i/8) + 1 runs, so the runs
// before row pair i = 8q + r number 4q(q+1) + r(q+1).
constexpr int FR_W = 4 * FT_W;
constexpr int FR_WAVES = 8;      // chain words (waves) per workgroup of the run kernel: 8 measured 46.5 us at cfg3, 16 54.4, 4 57.9
struct fpr_run {
    int n0, mb;
    int cnt0, cnt1;          // edges of row n0 / n0 + 1 in the run (m < n, row inside the triangle)
    int tile0, ntile;        // its pair-aligned tiles: tile0 .. tile0 + ntile - 1 (fpt_locate)
    int64_t cr0, cr1;        // edge id of the first column of each row
};
__host__ __device__ static inline int64_t fpr_runs(int64_t i) {        // runs of the row pairs before i
    const int64_t q = i >> 3;
    return 4 * q * (q + 1) + (i & 7) * (q + 1);
}
__host__ __device__ static inline fpr_run fpr_locate(int t, int Nreg) {
    int q = (int)((sqrtf((float)t + 1.f) - 1.f) * 0.5f);
    while ((int64_t)4 * (q + 1) * (q + 2) <= t) ++q;
    while ((int64_t)4 * q * (q + 1) > t) --q;
    const int rem = t - 4 * q * (q + 1);
    const int i = 8 * q + rem / (q + 1);
    fpr_run R;
    R.n0 = 2 * i;
    R.mb = FR_W * (rem % (q + 1));
    const int c0 = R.n0 - R.mb, c1 = R.n0 + 1 - R.mb;
    R.cnt0 = c0 < FR_W ? c0 : FR_W;
    R.cnt1 = R.n0 + 1 < Nreg ? (c1 < FR_W ? c1 : FR_W) : 0;
    R.tile0 = (int)fpt_tiles(i) + R.mb / FT_W;
    R.ntile = ((c1 + 1 < FR_W ? c1 + 1 : FR_W) + FT_W - 1) / FT_W;
    R.cr0 = ((int64_t)R.n0 * (R.n0 - 1) >> 1) + R.mb;
    R.cr1 = R.cr0 + R.n0;
    return R;
}
// the Philox blocks a run draws: per row the 4-id blocks its consecutive edge ids touch, each once
__host__ __device__ static inline int fpr_philox_blocks(const fpr_run &R) {
    int n = 0;
    if (R.cnt0 > 0) n += (int)(((R.cr0 + R.cnt0 - 1) >> 2) - (R.cr0 >> 2)) + 1;
    if (R.cnt1 > 0) n += (int)(((R.cr1 + R.cnt1 - 1) >> 2) - (R.cr1 >> 2)) + 1;
    return n;
}
// Pair records made once per call (fcd_gibbs.hip, gibbs_f_records_kernel): per pair-aligned tile NPAIR x FP_EC records of
// six 16-byte pieces (the eight of the LDS record without slots 10-11 and 14-15, which no slot word can name), then one
// fcd_f_edge_rec per edge id.
constexpr int F_REC_PIECES = 6;
struct fcd_f_edge_rec {
    double d1, d2;     // S_B[c][1] - S_B[c][0], S_B[c][2] - S_B[c][0]
    float a;           // bound of the sum over the patients of the largest |entry| of the row (the tile's B_e)
    float b[6];        // lo1, hi1, lo2, hi2, lo12, hi12 of fcd_f_edge_mode, rounded outward; NaN where a table entry is not finite
    float pad;
};
// An edge whose draw the tables decide.  The f pass's exact log-odds against type 0 are b_k = c_k + sum_u d_k(z_u), k = 1, 2:
// c_k = (ln gamma_k - ln gamma_0) + S_B[c][k] - S_B[c][0], (d_1, d_2)(z) = lMf[c][u][z][:], z_u in {typical, both, discordant}
// set by the r state.  With, over the patients,
//   lo1 = sum_u min_z d_1,  hi1 = sum_u max_z d_1,  lo2, hi2 likewise,  lo12 = sum_u min_z (d_1 - d_2),  hi12 = sum_u max_z (d_1 - d_2)
// (fp64, rounded outward: gibbs_f_records_kernel), type m leads the other two by more than T in EVERY r state if
//   m = 0:  -(c1 + hi1) > T  and  -(c2 + hi2) > T
//   m = 1:    c1 + lo1  > T  and    (c1 - c2) + lo12  > T
//   m = 2:    c2 + lo2  > T  and  -((c1 - c2) + hi12) > T
// -> m, or -1 (no such type; every comparison is false for a NaN, and an infinite c_k makes delta infinite).
// T = FCD_F_SURE_T = 16.  Let L be the exact lead, delta = fcd_f32_sum_err + fcd_f32_offset_err the edge's bound on |bf_k - b_k| of
// the term loop's fp32 sums, M = max |bf_k| <= cm + a + delta, u = 2^-24.  (1) L > 15: fcd_draw_f_sure's argument holds for the
// exact sums, fcd_draw_f returns the argmax for x in [1e-6, 1 - 1e-6].  (2) fcd_draw_f_sure computes (mx - mid) - eta from the
// fp32 sums: the lead among (0, bf1, bf2) is >= L - 2 delta; mid = ((bf1 + bf2) - mx) - mn rounds three times (2uM, 3uM, uM),
// mx - mid and - eta once each (2uM, u(2M + eta)): together < 10.1 uM <= 6.1e-7 (cm + a + delta) <= 5.1 delta, because
// delta >= fcd_f32_offset_err = 1.2e-7 (cm + a).  So the test passes, with the fp32 argmax the exact one, where
// L > 15.01 + eta + 7.1 delta.  An edge counts only with delta <= FCD_F_SURE_DELTA_CAP = 1/32, which caps
// eta = fcd_draw_f_eta(delta) <= expm1(1/16) 1.001 + 2e-5 < 0.065: 15.01 + 0.065 + 0.222 = 15.30.  The rest of T covers the
// fp64 roundings of c_k + bound (1.2e-16 relative, of magnitudes that keep delta under its cap: < 1e-10).
// tests/test_f_sure_rule.py restates the rule in NumPy.
#define FCD_F_SURE_T 16.0
#define FCD_F_SURE_DELTA_CAP 0.03125f
#define FCD_F_SURE_DRIFT 6.0      // the table's hint (fcd_ctx::hint) uses T - this: gamma moves with the M-steps of a call
__host__ __device__ static inline int fcd_f_edge_mode(double c1, double c2, const float *b, float delta, double T) {
    if (!(delta <= FCD_F_SURE_DELTA_CAP)) return -1;
    const double c12 = c1 - c2;
    if (-(c1 + (double)b[1]) > T && -(c2 + (double)b[3]) > T) return 0;
    if (c1 + (double)b[0] > T && c12 + (double)b[4] > T) return 1;
    if (c2 + (double)b[2] > T && -(c12 + (double)b[5]) > T) return 2;
    return -1;
}
// (c1, c2, delta) of an edge from its record and the sweep's hyper, as the pair-tile kernel makes its constants
__host__ __device__ static inline float fcd_f_edge_delta(double c1, double c2, int NPAIR, float a) {
    const float cm = fmaxf((float)fabs(c1), (float)fabs(c2)) * 1.0000002f;
    return fcd_f32_sum_err(NPAIR, a) + fcd_f32_offset_err(cm, a);
}
constexpr size_t F_REC_CAP = (size_t)256 << 20;     // no record table above this many bytes: the tiles build their own
// A call of the sweep loop makes the records where it has at least this many pair-tile sweeps: the build launch costs 27.4 us
// at cfg3 and a pair-tile f pass on its records runs 6.75 us shorter (108.96 -> 102.20 us; kernel trace of the timed loop,
// profiles/f_records_per_call_cfg3.txt), so it is paid back after ceil(27.4 / 6.75) = 5 sweeps -- doubled.
constexpr int F_REC_MIN_SWEEPS = 10;
struct fcd_sweep_plan {
    int f_form, f_EC;           // f pass given lMf: form, edges per LDS tile
    size_t f_shmem;
    int f_NW;                   // slot-source words per region (pack_ru_word) the pair forms read, pack_ru / the tally make
    bool r_blocked, r_idx32;    // r pass given lMd: the blocked form fits; its item indices fit 32 bits (else it refuses)
    int r_ub;                   // ... patients per panel workgroup
    size_t r_shmem;
    // square copy of the f state (fcd_ctx::fsq, (GW,Nreg,Nreg,64) u8) a pair-form f pass writes and the r pass packs
    // from (contiguous rows instead of 64-byte pieces); 0: none
    size_t fsq_bytes;
    // prebuilt pair records of the pair-tile f pass (fcd_ctx::frec): tiles | edge constants at frec_edge; 0: none (another
    // form, no blocked r pass, or above F_REC_CAP).  f_shmem_rec: the LDS of the kernel that reads them (no fp64 rows)
    // frec_votes: behind the edge constants one word per (run, group of 16 chain words), zero between passes -- where the two
    // 8-wave workgroups of such an item meet for the counters (gibbs_f_run_kernel)
    size_t frec_bytes, frec_edge, frec_votes, f_shmem_rec;
    // workspace byte offsets: P[0] | P[1] | f_S | r_S | r_Sn | marks of the blocked r pass, then at a 512-byte boundary the
    // slot words r_U of a pair-form f pass (behind the r scratch: the sentinels in P survive from sweep to sweep) | ws_bytes
    size_t P[2], f_S, r_S, r_Sn, marks, r_U, ws_bytes;
    // the sparse r pass's per-call tables and per-pass words, behind the slot words (rs_bytes == 0: none -- no record table):
    // bounds hi | lo (Nreg, U) fp64, the rows of differences (U, Nreg, Nreg) fp64 with base(n,u) on the diagonal, mode words
    // (Nreg, NBLK) uint2, row flags (Nreg) u32, then per pass the sites to visit (GW, Nreg) u64 over u and "the row's f words
    // differ from the modes" (GW, Nreg) u32
    size_t rs_bnd, rs_dtab, rs_mword, rs_rowflag, rs_visit, rs_fneq, rs_bytes;
};
fcd_sweep_plan fcd_sweep_plan_for(const fcd_ctx *ctx, int64_t Nreg, int64_t U, int64_t GW);
// one call of a sweep entry point; fcd_sweep_call_check (fcd_gibbs.hip) checks it and fills in g and pl
struct fcd_sweep_call {
    const double *S_B, *lM, *lMf, *lMd, *hyper;
    uint8_t *f_state;
    uint64_t *r_bits;
    int64_t Nreg, U, G, chain0;
    uint64_t seed;
    int edge_mode;
    hipStream_t s;
    fcd_geo g;
    fcd_sweep_plan pl;
};
int fcd_sweep_call_check(fcd_ctx *ctx, fcd_sweep_call &c, bool f_pass, bool r_pass, const char *who);
// what changes from one sweep of a call to the next
struct fcd_sweep_step {
    int64_t sweep;
    uint8_t *fsq;                  // square copy of the f state, or nullptr
    bool f_packed;                 // f pass: write the r pass's f words (f_S) in their final form (pair tiles), no square copy
    bool r_packed;                 // r pass: r_S holds the r words (the previous pass wrote them, or the tally made them) and the
                                   // previous sweep's tally has cleared the marks
    bool ru_ready;                 // f pass: the previous sweep's tally has made the slot words
    const void *f_rec;             // f pass (f_packed): pair records made for this call, or nullptr (the tiles build their own)
    bool sentinels_in_place;       // r pass: P holds the sentinels a COMPLETED pipelined pass of this shape left behind
    const fcd_tally_f *tally_f;    // f and r pass: the f half of the tally to carry in the run kernel, the packing launch or the
    bool tally_f_done;             // pipelined launch, or nullptr ... and whether one of them did (cleared by the sweep loop, set by the carrier)
    bool f_fold;                   // r pass: the run kernel has left the pooled f counts in fcd_ctx::f_slots; fold them into acc
    bool r_flip;                   // r pass: the two r-word buffers of the plan have swapped roles (r_S lies at pl.r_Sn, r_Sn at pl.r_S)
    bool f_sure;                   // f pass (f_rec): some tile of the call's table has all its edges decided (fcd_ctx::hint)
    bool f_all;                    // ... and every tile has: the decided path runs in its run form (gibbs_f_run_kernel)
    bool r_sure;                   // r pass: the sparse form (the call's site bounds are built and the rule of the knob r_sure chose it)
};
int fcd_gibbs_f_pass(fcd_ctx *ctx, const fcd_sweep_call &c, fcd_sweep_step &st);         // fcd_gibbs.hip
int fcd_gibbs_r_pass(fcd_ctx *ctx, const fcd_sweep_call &c, fcd_sweep_step &st);         // fcd_gibbs_r.hip
// Decided sites of the r pass (fcd_gibbs_r.hip, gibbs_r_sparse_kernel).  With the edge modes k* of fcd_f_edge_mode at the call's
// starting hyper and T - FCD_F_SURE_DRIFT, the log-odds of r_nu = 1 are  off + sum_{m != n} lMd[u][n][m][f_nm][r_m],
// off = ln pi - ln(1 - pi).  Where every edge of row n has a mode and every f_nm equals it,
//   lo(n,u) = sum_m min_t lMd[u][n][m][k*][t]  <=  sum  <=  hi(n,u) = sum_m max_t lMd[u][n][m][k*][t]
// in every r state.  The site is decided 0 iff hi + off < -R_SURE_T, decided 1 iff lo + off > R_SURE_T: logit(x) >= -13.82
// for x >= 1e-6, so  logit(x) < v  is false (true) for every x in [1e-6, 1 - 1e-6]; the 2.18 nats in hand cover the outward
// rounding of the bounds, the fp64 error of the kernels' own sums and FCD_LOGIT_FAST_ERR.  The share of decided sites from
// which the sparse form is chosen: see DESIGN.md, "Decided sites of the r pass".
#define R_SURE_T 16.0
#define R_SURE_X 1e-6
// Measured at Nreg 200, U 50, 1024 chains with the tables scaled by beta (ms per sweep, pipelined form against sparse form, share
// of the (site, word) items the passes left to the tables): beta 1: 0.289 / 0.151 (0.949); 0.5: 0.289 / 0.198 (0.931);
// 0.35: 0.289 / 0.335 (0.769); 0.3: 0.289 / 0.427 (0.523); H = 20 controls, where one row in ten has an edge without a mode and
// is walked in full: 0.314 / 0.461 (0.869).  The sparse form wins at 0.93 and loses at 0.87 and below.
constexpr double R_SURE_MIN_SHARE = 0.9;
// the bound build and its hint (queued by the sweep loop once the f hint says that some tile is decided)
int fcd_gibbs_r_bounds_build(fcd_ctx *ctx, const fcd_sweep_call &c);

// ---------------------------------------------------------------------------------------------
// Ablation build (make ABLATE=1 -> libfcdiff_hip_abl.so, NEVER the product library): kernels read a level
// from device memory and skip parts of their work so that phases can be timed A/B in one process.
// Results are wrong whenever the level is non-zero.  In the product build FCD_ABL(x) folds to false.
// ---------------------------------------------------------------------------------------------
#ifdef FCD_ABLATE
extern __device__ int fcd_abl_level[4];   // [0] f kernel, [1] panel, [2] diag, [3] row stamps of the pipelined scan
#ifdef FCD_TRACE_ONLY     // (make ABLATE=1 TRACE_ONLY=1: the time stamps without the ablation switches -- the product's code otherwise)
#define FCD_ABL(slot, lvl) false
#else
#define FCD_ABL(slot, lvl) (fcd_abl_level[slot] >= (lvl))
#endif
void fcd_abl_refresh(hipStream_t s);
// Timeline of the r step kernel: record (launch, workgroup) x 8 words of the 100 MHz clock, written by thread 0
// when FCD_TRACE_PTR names a device buffer (profiles/trace_r.py).
extern __device__ unsigned long long *fcd_trace_buf;
#define FCD_TRACE(rec, slot)                                                                      \
    do {                                                                                          \
        if (fcd_trace_buf && threadIdx.x == 0) fcd_trace_buf[(size_t)(rec) * 8 + (slot)] = wall_clock64(); \
    } while (0)
#define FCD_TRACE_VAL(rec, slot, v)                                                               \
    do {                                                                                          \
        if (fcd_trace_buf && threadIdx.x == 0) fcd_trace_buf[(size_t)(rec) * 8 + (slot)] = (unsigned long long)(v); \
    } while (0)
// the same from thread t0 of the workgroup
#define FCD_TRACE_AT(t0, rec, slot)                                                               \
    do {                                                                                          \
        if (fcd_trace_buf && threadIdx.x == (t0)) fcd_trace_buf[(size_t)(rec) * 8 + (slot)] = wall_clock64(); \
    } while (0)
#define FCD_TRACE_VAL_AT(t0, rec, slot, v)                                                        \
    do {                                                                                          \
        if (fcd_trace_buf && threadIdx.x == (t0)) fcd_trace_buf[(size_t)(rec) * 8 + (slot)] = (unsigned long long)(v); \
    } while (0)
#else
#define FCD_ABL(slot, lvl) false
#define FCD_TRACE(rec, slot) do { } while (0)
#define FCD_TRACE_VAL(rec, slot, v) do { } while (0)
#define FCD_TRACE_AT(t0, rec, slot) do { } while (0)
#define FCD_TRACE_VAL_AT(t0, rec, slot, v) do { } while (0)
static inline void fcd_abl_refresh(hipStream_t) {}
#endif
