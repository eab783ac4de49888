/*
 * fcdiff_hip.h -- C ABI of libfcdiff_hip.so, the MI355X (gfx950) implementation of the fcdiff
 * fit path.  Plain C: raw device pointers, sizes, a hipStream_t passed as void*.  No torch, no
 * C++ types.  Every function returns 0 on success, a negative FCD_ERR_* for an argument error
 * detected on the host, or a positive hipError_t.  Nothing throws; nothing synchronises the
 * device or allocates unless its comment says so (fcd_ctx_create / fcd_ctx_destroy / fcd_ctx_reserve do; any
 * sampler or fit entry point does ONLY when it meets a shape larger than fcd_ctx_reserve was told: it then grows
 * the context's scratch once, which is a hipDeviceSynchronize + hipMalloc -- fcd_ctx_stat "n_alloc" counts them).
 * There is no global state: all of it sits behind fcd_ctx.  No entry point reads the environment; the tuning /
 * test knobs take their defaults from it once, in fcd_ctx_create.
 *
 * The reference (andy-sweet/fcdiff) is pure Python/NumPy and has NO native interface; what each
 * entry point replaces is therefore a NumPy method of fcdiff/fit.py, cited per function.  The
 * binding a maintainer would add on the reference side is a ctypes stub.
 *
 * Naming follows the reference: Nreg regions ("N" there), C = Nreg(Nreg-1)/2 edges in
 * lower-triangular row-major order c = n(n-1)/2 + m, n > m (fcdiff/util.py:40-84), H healthy
 * subjects, U patients.  All floating point is IEEE binary64.
 *
 * Array layouts (all C-contiguous, device memory unless marked "host"):
 *   b        (C, H)        correlations of healthy subjects          fcdiff/fit.py:20-21
 *   bt       (C, U)        correlations of patients                  fcdiff/fit.py:22-23
 *   S_B      (C, 3)        sum_h log N(b[c,h]; mu_k, sigma_k): the H-sum of _lp_B_g_F, which is all
 *                          fit.py:171 and :472 ever consume
 *   lM       (C, U, 3, 3)  _lM[c,u,k,l], the reference's layout       fcdiff/fit.py:48-49
 *   lq_F     (C, 1, 3)     _lq_F                                     fcdiff/fit.py:42-43
 *   lq_R     (Nreg, U, 2)  _lq_R                                     fcdiff/fit.py:40-41
 *   hyper    (8,)          {ln gamma_0..2, ln(1-pi), ln pi, 0, 0, 0}: the hyper-parameters every
 *                          conditional reads; lives on the device so an M-step never needs the host
 *   theta    (12,) host    {pi, eta, epsilon, gamma[3], mu[3], sigma[3]}  fcdiff/model.py:31-38
 * Chain state of the Gibbs sampler, G chains padded to GW = ceil(G/64) words of 64 chains:
 *   f_state  (GW, C, 64)   uint8 in {0,1,2}: f_c of chain 64*w + lane at [(w*C + c)*64 + lane]
 *   r_bits   (GW, Nreg, U) uint64: bit `lane` of [(w*Nreg + n)*U + u] is r_{n,u} of chain 64*w+lane
 *
 * ALIGNMENT of device pointers.  Every device pointer must be aligned to its element type (8 bytes for double, int64_t
 * and uint64_t, 4 for the 32-bit types, 2 for uint16_t).  The pointers listed below must be 16-byte aligned as well: their
 * kernels read or write them as 16-byte (f_state in two places: 4-byte) vectors, and nothing narrower is built.  A
 * violation is refused on the host, before any launch, with FCD_ERR_ARG and the message
 * "<entry point>: argument <name> must be 16-byte aligned"; a null pointer passes this check (each entry point says which
 * of its pointers may be null).  A buffer from hipMalloc or from PyTorch's allocator always qualifies; a slice of one, or
 * a table packed into an arena at an odd number of doubles, may not.  DESIGN.md ("Alignment of caller pointers") has the
 * access behind every line, and tests/test_alignment_contract.py reads this list:
 *   align16: fcd_lik_tables(lM)
 *   align16: fcd_lik_tables_ex(lM)
 *   align16: fcd_lik_tables_sessions(lM)
 *   align16: fcd_lik_tables_noise(lM)
 *   align16: fcd_corr_edges(ts)                           when T is even
 *   align16: fcd_corr_partial(ts)                         when T is even
 *   align16: fcd_tangent_fit(ts)                          when T is even
 *   align16: fcd_tangent_apply(ts)                        when T is even
 *   align16: fcd_gibbs_f_step(f_state, lMf)
 *   align16: fcd_gibbs_r_step(f_state, lMd)
 *   align16: fcd_gibbs_sweeps(f_state, lMf, lMd)
 *   align16: fcd_gibbs_run(f_state, lMf, lMd)
 *   align16: fcd_gibbs_tally(f_state)
 *   align16: fcd_gibbs_stats(f_state)
 *   align16: fcd_gibbs_accumulate(f_state)
 *   align16: fcd_score_ais_step(f_state)
 * Three entry points choose their path by the address and take element-aligned pointers at full correctness, 16-byte
 * ones faster; their own comments say so:
 *   by-address: fcd_edge_cov_apply(x, out)
 *   by-address: fcd_site_harmonize_apply(x, out)
 *   by-address: fcd_evidence_temper(src, dst)
 * Every other pointer of every entry point is read and written one element at a time.
 */
#ifndef FCDIFF_HIP_H
#define FCDIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCD_ABI_VERSION 4

#define FCD_OK 0
#define FCD_ERR_ARG (-1)         /* null pointer / non-positive size */
#define FCD_ERR_SHAPE (-2)       /* C is not a triangular number (fit.py:62-65), Nreg < 2, ... */
#define FCD_ERR_UNSUPPORTED (-3) /* shape outside what the kernels are built for (message says which) */
#define FCD_ERR_INDEX (-4)       /* reference edge ids run out of range (Nreg == 2, fit.py:186) */
#define FCD_ERR_DEVICE (-5)      /* a kernel gave up a device-side wait (one-launch r pass); the chain state is unusable */
#define FCD_ERR_COMM (-6)        /* RCCL: library not found, or a call failed (fcd_last_message says which) */
#define FCD_COMM_ID_BYTES 128    /* sizeof(ncclUniqueId) */

/* Edge id used by the region update for an ordered pair (n, m), m != n. */
#define FCD_EDGE_REFERENCE 0 /* nm_to_c(n,m) = n(n-1)/2 + m for EVERY ordered pair, as fit.py:185-186 calls it */
#define FCD_EDGE_SYMMETRIC 1 /* the unordered pair's edge, as doc/methods.rst:646-653 writes it */

/* `flags` of the *_ex entry points: how b / bt are read.
 * FCD_DATA_NAN_MISSING: a NaN entry of b or bt is unobserved and is integrated out.  The fitter's densities of b and bt
 * are plain Normals (no clip to [-1, 1]) and each integrates to 1, so a NaN b[c,h] adds 0 to S_B[c,k] for every k and a
 * NaN bt[c,u] has N_j = 1 for every j, M_kl = 1 and lM[c,u,k,l] = 0.  Only NaN is missing (+-inf is read as a value).
 * Every other entry point reads the data only through S_B and lM and needs no flag.  flags = 0: the plain entry points'
 * results, bit for bit (they are the flags = 0 forms). */
#define FCD_DATA_NAN_MISSING 1
/* FCD_W_PER_EDGE (fcd_theta_sub_objective_ex, fcd_theta_full_objective_ex only): W is (C, 1, 3, 3), one weight table per
 * edge that every patient's bt[c, u] is weighted with -- the shared-region model, whose weights do not depend on u. */
#define FCD_W_PER_EDGE 2

typedef struct fcd_ctx fcd_ctx;
typedef void *fcd_stream; /* hipStream_t */

int fcd_abi_version(void);
/* Static string for any return code of this library (hipGetErrorString for positive codes). */
const char *fcd_strerror(int code);
/* Last host-side diagnostic of this ctx (which argument / which limit); never NULL. */
const char *fcd_last_message(const fcd_ctx *ctx);

/* Context on the CURRENT hip device: reduction workspace + device properties.  create/destroy
 * allocate/free device memory (they synchronise); nothing else does, except that a call needing a
 * larger workspace than any before grows it (hipDeviceSynchronize + hipMalloc) -- call fcd_ctx_reserve
 * first to avoid that.
 * Streams: every device entry point queues ALL of its work (launches, memsets, copies) on the fcd_stream it is given and
 * returns without waiting for it, unless its comment says otherwise.  A context serves ONE stream at a time: its workspace,
 * tickets and accumulators are shared by all of its calls, so consecutive calls on DIFFERENT streams need the caller's own
 * ordering between them (an event or a synchronisation); calls on one stream need none.  Any number of contexts may run
 * side by side, each on a stream of its own: there is no process-wide device state.  Growth of a context's scratch
 * synchronises the DEVICE, every stream of it (stat "n_alloc" counts the growths). */
int fcd_ctx_create(fcd_ctx **out);
int fcd_ctx_destroy(fcd_ctx *ctx);
/* Sizes every scratch buffer of the sweep at this shape (f / r pass workspace, square f copy) from the same plan the
 * sampler entry points read (shape and knobs): after it none of them allocates or synchronises at shapes up to
 * (Nreg, U, G) while the knobs stay as they are.  Synchronises when it grows something. */
int fcd_ctx_reserve(fcd_ctx *ctx, int64_t Nreg, int64_t U, int64_t G);
/* Tuning / test knobs (defaults: environment FCD_R_PATH, FCD_R_UB, FCD_R_NOPAD, FCD_R_DSPLIT, FCD_R_COOP, FCD_R_REFILL, FCD_R_TOL, FCD_F_TOL, FCD_F_FORM,
 * FCD_F_PACK, FCD_CORR_FORM, FCD_TALLY_IN_R, FCD_R_KEEP_WORDS, read once by fcd_ctx_create; 0 = default everywhere; the two test hooks at the end of the list are NOT read
 * from the environment -- a stray variable must not be able to make a fit give up):
 *   "r_path"    0: blocked r pass in its pipelined one-launch form (marks / sentinels in device memory instead of
 *                  kernel boundaries) wherever every workgroup is resident at once, else one launch per block step;
 *               3: one launch per block step always
 *   "r_ub"      1 / 2 / 4: patients per panel workgroup of the blocked r pass (0: chosen by shape)
 *   "r_nopad"   1: no empty workgroups beside the in-order workgroups
 *   "r_dsplit"  1: ONE in-order workgroup per patient in the pipelined r pass (default: two, 8 chain words each, on two CUs,
 *               where a group has more than 8 chain words and 2 U <= number of CUs)
 *   "r_coop"    1: COOPERATIVE launch of the pipelined r pass -- the runtime itself checks that the grid is resident at once
 *               and the pass falls back to one launch per block step if it refuses (measured +16 us per pass at cfg3, so
 *               not the default; the default relies on the occupancy query, 8 spare slots and bounded polls)
 *   "r_refill"  1: the pipelined r pass's packing launch writes the panel-value sentinels in every sweep (default: only in the
 *               first sweep of a fcd_gibbs_run call -- a completed pass leaves every slot holding its sentinel again)
 *   "qr_form"   fcd_vb_update_qR: 1 = operands gathered from the edge-major table inside the region loop (rounds 1-3; the
 *               default where the region-major weights would exceed 192 MB: cfg5), 2 = region-major weights made first
 *               whatever their size (the default below that: cfg3)
 *   "corr_form" 1: fcd_corr_edges in 64 x 64 blocks with a moments pass also where the one-workgroup-per-subject kernel
 *               (up to 208 regions) would run
 *   "partial_chunk"  > 0: fcd_corr_partial walks at most this many subjects per chunk (tests; not read from the environment)
 *   "tangent_chunk"  > 0: the same for fcd_tangent_fit and fcd_tangent_apply, and at most this many matrices per launch of
 *               fcd_sym_eigh
 *   "r_tol", "f_tol"  widen the margin inside which a fast r / f draw is repeated with the exact formula (1e30: all)
 *   "f_form"    2: the any-U pair kernel of the f pass also where the U <= 64 kernel would run; 3: scalar-mask form
 *   "f_pack"    1: the r pass's packing launch in every sweep (default: from the second sweep of a fcd_gibbs_run call on,
 *               the U <= 64 f pass writes the r pass's packed f words itself and the tally the r words of the next pass)
 *   "f_records" the pair-tile f pass (U <= 64, every sweep of a fcd_gibbs_run / fcd_gibbs_sweeps call but the first) reads
 *               pair records and edge bounds that one launch makes for the whole call, instead of building them in every
 *               tile: 0 = in calls with at least F_REC_MIN_SWEEPS such sweeps (stat "f_rec_min_sweeps"), 1 = never, 2 = in
 *               every call that has one (A/B runs and tests; not read from the environment).  The table (stat
 *               "f_rec_bytes") belongs to the context, fcd_ctx_reserve sizes it; above 256 MB, or where the device has no
 *               room for it, the tiles build their own records
 *   "f_sure"    1: never the decided-tile path of the pair-tile f pass on those records (default: in calls whose table has a
 *               tile with every edge decided by the tables -- the mode leads by more than 16 nats in every r state -- such
 *               tiles draw their Philox words, test them against the range of the draw without exponential and, if every lane
 *               of the workgroup is inside, write the modes: no sums.  A/B runs and tests; not read from the environment)
 *   "f_runs"    the form of that path: 0 = where the record build finds EVERY tile decided, one wave per (block-wide run of up
 *               to four tiles, chain word) draws each Philox block of a row once, writes the modes with 16- and 8-byte stores
 *               and draws by itself the few edges for which one of its lanes is out of range (no workgroup-wide vote, no tile
 *               goes back as a whole); elsewhere the per-tile kernel; 1 = never the run form; 2 = the run form wherever the
 *               path is taken at all (tests: edges the rule leaves open are then drawn inside the run kernel).  Not read
 *               from the environment
 *   "r_sure"    the sparse form of the r pass on a call's record table (knob f_records' gate): a site whose draw the tables
 *               decide -- with every edge of its row at its mode the log-odds of r = 1 stay below -16 (above 16) in every r
 *               state -- gets its r word from a range test of its uniform, the other sites are walked in order with sums of a
 *               few terms.  0 = in calls whose bound build finds at least nine tenths of the sites decided (and only with "r_tol" at
 *               its default and "r_path", "r_coop", "r_dsplit" unset), 1 = never, 2 = wherever the bounds exist (tests).  Not
 *               read from the environment
 *   "r_sure_x"  TEST HOOK: > 1e-6 widens the range of uniforms that sends a decided site to the full evaluation (0.25: half
 *               of all draws)
 *   "tally_in_r" the f half of a sweep's tally (pooled counts of f, cnt_f) inside the pipelined r pass, counted by its in-order
 *               workgroups before their first block, while they wait for the first panel values: 0 = where those workgroups
 *               have 16 waves and a wave walks at most "tally_in_r_max_rounds" rounds of four edges (cfg3: 4 rounds), 1 = never
 *               (the tally launch after the pass counts f), 2 = wherever the workgroups have 16 waves.  The packing launch
 *               of a call's first sweep keeps the f half it carries (stat "tally_f_in_pack"); the step-per-launch form carries none
 *   "tally_in_f" the f half of a sweep's tally counted by the f pass's run kernel as it stores its draws (no pass reads the f
 *               state back): 0 = in sweeps whose r pass is sparse (nothing else then carries it), 1 = never, 2 = wherever the
 *               run form runs (tests).  Not read from the environment
 *   "r_keep_words" 1: the tally makes the next r pass's r words from the r bits (default: inside a fcd_gibbs_run /
 *               fcd_gibbs_sweeps call the pass's two r-word buffers swap roles from sweep to sweep -- the words a pass wrote
 *               are the next pass's -- and the tally only clears the marks)
 *   "r_poll_limit", "r_withhold"  TEST HOOKS of the pipelined r pass: bound every device-side poll by this many polls /
 *               the in-order role never announces a block (a panel wave then gives its wait up, fcd_ctx_check reports it)
 *   "r_coop" = 2  TEST HOOK: every pipelined launch of the r pass acts as if the runtime had refused a cooperative launch
 *               (it launches nothing, and the pass falls back to one launch per block step); FCD_R_COOP=2 means 0
 * None of them changes a result: every combination walks the same chains (tests/test_gpu_parity.py).
 * (Round 2 carried eight more forms behind knobs -- a one-launch form with counters, a row-sequential kernel, two-stream
 * half-passes, a pair-record table, triple records in the f pass, ... -- all measured slower; DESIGN.md keeps the numbers.) */
int fcd_ctx_set_knob(fcd_ctx *ctx, const char *name, double value);
/* Counters of the context: "n_alloc" device allocations made so far, "ws_bytes", "fsq_bytes"; "r_form_last" = the form
 * the last blocked r pass ran in (1 one launch per block step, 2 pipelined one-launch form, 3 one-launch form with
 * counters); "pack_launches" = packing launches of the r pass made so far; "tally_f_in_pack" = those of them that also
 * carried the f half of the sweep's tally; "tally_f_in_r" = launches of the pipelined r pass that carried it,
 * "tally_f_in_f" = f passes whose run kernel counted it (knob tally_in_f; no sweep is counted by two of the three),
 * "tally_in_r_max_rounds" = the threshold of knob tally_in_r = 0; "f_rec_passes" = f passes that read prebuilt pair records, "f_rec_builds" =
 * launches of the kernel that makes them, "f_rec_bytes" = the size of their table, "f_rec_min_sweeps" = the threshold of
 * knob f_records = 0; "f_sure_passes" = f passes that ran a kernel with the decided-tile path, "f_run_passes" = those of them in
 * the run form (knob f_runs), "f_sure_tiles" = (pair-aligned tile x 16 chain words) items that took it, "f_sure_fallbacks" = decided
 * ones in which a uniform outside the range sent the tile (run form: only that wave's edge) back to
 * the sums (the last two and "f_repeats", "r_exact_rows" are device counters: reading them synchronises);
 * "r_form_last" = 4: the sparse form (knob r_sure); "r_sure_passes" = r passes in that form, "r_sure_builds" = launches of the
 * kernel that makes its bounds (once per call, and only where the f pass's hint says that some tile is decided),
 * "r_sure_sites" = (site, 64-chain word) items such passes left to the tables, "r_sure_exceptions" = decided items they
 * evaluated in full all the same -- a uniform out of range in some chain, or the row's f off its modes (device counters);
 * "dev_err" = the error word of the pipelined r pass as the host sees it now (see
 * fcd_ctx_check); "pipe_grid" / "pipe_capacity" = the grid of the last pipelined attempt of the r pass (its empty
 * workgroups included) and the workgroups the occupancy query says are resident at once for it (the form is taken where
 * pipe_grid + 8 <= pipe_capacity). */
int fcd_ctx_stat(const fcd_ctx *ctx, const char *name, int64_t *out);
/* FCD_ERR_DEVICE if a kernel of this context has abandoned a device-side wait (pipelined r pass: every poll of a mark or
 * of a panel value is bounded, ~1 s), else FCD_OK.  The word is written by the device: call this AFTER the stream has been
 * synchronised (or after any device-to-host read that follows the sweeps on that stream) -- the sampler entry points
 * themselves only see a give-up of an EARLIER call.  Once set, the chain state is unusable; fcd_ctx_clear_error resets
 * the word after the caller has re-initialised its chains, and puts the context-owned accumulators and tickets (pooled
 * counts of the tally, K_corr's per-subject tickets) back to zero (it synchronises: an error-recovery call). */
int fcd_ctx_check(fcd_ctx *ctx);
int fcd_ctx_clear_error(fcd_ctx *ctx);

/* ---- the one exchange between GPUs: pooled counts before a (pi, gamma) M-step --------------------------------------
 * ("fcd_allreduce_stats(ncclComm_t, ...)"; the reference has no counterpart -- single process.)
 * One process per GPU.  The communicator belongs to the context and is made ONCE, before any sweep:
 *   fcd_comm_load(ctx, path)     take RCCL's entry points from the librccl the process already holds (path = the file the
 *                                host framework loaded, e.g. <torch>/lib/librccl.so; NULL / "" tries librccl.so.1)
 *   fcd_comm_unique_id(ctx, id)  rank 0: ncclGetUniqueId -> 128 bytes, broadcast to the other ranks by whatever the caller
 *                                has (the Python mirror uses its torch.distributed group)
 *   fcd_comm_init(ctx, id, world, rank)   every rank (collective): ncclCommInitRank
 * From then on fcd_gibbs_run pools the counts of every M-step over the communicator's ranks with ncclAllReduce(8 x int64,
 * sum) ON THE STREAM OF THE SWEEP KERNELS, between the tally and a one-thread M-step kernel: no copy of the counts, no
 * event between streams, no host in the loop.  A communicator of one rank is legal (and tested on the one-GPU box).
 * fcd_allreduce_stats does the same for a caller-owned counts vector (8 int64, device), e.g. after fcd_gibbs_stats.
 * fcd_comm_destroy before fcd_ctx_destroy (which also calls it). */
int fcd_comm_load(fcd_ctx *ctx, const char *librccl_path);
int fcd_comm_unique_id(fcd_ctx *ctx, uint8_t *id128);
int fcd_comm_init(fcd_ctx *ctx, const uint8_t *id128, int world, int rank);
int fcd_comm_destroy(fcd_ctx *ctx);
int fcd_allreduce_stats(fcd_ctx *ctx, int64_t *counts, fcd_stream stream);

/* Optional timing of the library's main kernels with HIP events recorded on the launch stream, each pair
 * bracketing exactly ONE kernel launch.  slot: 0 likelihood tables, 1 f pass, 2 r block step (or one-launch pass), 3 r pack.
 * fcd_prof_collect waits for the recorded events, returns the summed milliseconds and the number of
 * launches, and clears the slot.  Off by default (no events are recorded). */
int fcd_prof_enable(fcd_ctx *ctx, int on);
int fcd_prof_collect(fcd_ctx *ctx, int slot, double *total_ms, int64_t *count);

/* ---- index maps: fcdiff/util.py:7-84 (host, integer) ------------------------------------- */
int64_t fcd_N_to_C(int64_t Nreg);
/* Returns Nreg with C = Nreg(Nreg-1)/2, or FCD_ERR_SHAPE when C is not triangular (fit.py:62-65). */
int64_t fcd_C_to_N(int64_t C);
int64_t fcd_nm_to_c(int64_t n, int64_t m);
int fcd_c_to_nm(int64_t c, int64_t *n, int64_t *m);
/* The block-wide runs of the f pass's decided path (knob "f_runs"): fcd_f_run_count = their number at Nreg regions;
 * fcd_f_run_locate writes run t's out[0..8] = first row n0 (rows n0, n0 + 1), first column, edges of row n0 and of row n0 + 1,
 * first pair-aligned tile, number of tiles, edge id of each row's first column, and the Philox blocks the run draws. */
int64_t fcd_f_run_count(int64_t Nreg);
int fcd_f_run_locate(int64_t Nreg, int64_t t, int64_t *out9);

/* ---- hyper-parameter block ---------------------------------------------------------------- */
/* Writes hyper[0..7] from host values: gamma[3] and the 2-vector pi2 = {1-pi, pi} the reference
 * indexes (quirk Q4: fit.py:183, :486; test_fit.py:208, 477-487).  Asynchronous on `stream`. */
int fcd_hyper_set(fcd_ctx *ctx, double *hyper, const double *gamma3_host, const double *pi2_host,
                  fcd_stream stream);

/* ---- likelihood tables: UnsharedRegionFit._update_lps, fit.py:104-122 + _eval_M 409-444 ----
 * Same arithmetic as the reference: linear-space Normal densities, M_kl = eps_l N_k +
 * (1-eps_l)/2 sum_{j!=k} N_j, lM = log M (so a fully underflowed density gives -inf exactly as
 * there).  lp_B_g_F (C,H,3) and p_Bt_g_Ft (C,U,3) are written only when non-NULL (the fit path
 * never reads them; the Python mirror exposes them lazily).
 * Alignment: lM must be 16-byte aligned (ALIGNMENT, top of this file). */
int fcd_lik_tables(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                   const double *theta12_host, double *S_B, double *lM, double *lp_B_g_F,
                   double *p_Bt_g_Ft, fcd_stream stream);
/* fcd_lik_tables with flags.  With FCD_DATA_NAN_MISSING: S_B[c,k] sums over the observed h only, lM[c,u,:,:] = 0.0
 * exactly at a NaN bt[c,u]; lp_B_g_F holds 0.0 at a NaN b and p_Bt_g_Ft 1.0 at a NaN bt.  n_missing2 (device, int64[2],
 * may be NULL; only with the flag) receives {number of NaN in b, number of NaN in bt}, counted by
 * the table kernel (one atomic per block, into the context's slots) and written by one more small launch on `stream`.
 * Asynchronous like every table build.
 * Alignment: lM must be 16-byte aligned (ALIGNMENT, top of this file). */
int fcd_lik_tables_ex(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                      const double *theta12_host, double *S_B, double *lM, double *lp_B_g_F, double *p_Bt_g_Ft,
                      int flags, int64_t *n_missing2, fcd_stream stream);
/* The tables of the shared-region model (SharedRegionFit): S_B (C,3) as fcd_lik_tables writes it, bit for bit, and the
 * patient sum L (C,3,3), L[c,k,l] = sum_u lM[c,u,k,l], in ONE launch that reads b and bt once and writes nothing of size
 * C*U.  Per item the arithmetic of fcd_lik_tables; the sum over u has a fixed order (no atomics): two calls agree bit
 * for bit.  flags as fcd_lik_tables_ex: with FCD_DATA_NAN_MISSING a NaN bt adds 0 to L, a NaN b 0 to S_B, and
 * nan_counts (device int64[2], may be NULL; only with the flag) receives {NaN in b, NaN in bt}.  Without it a NaN
 * gives NaN.  An underflowed density gives -inf in L as in lM. */
int fcd_lik_shared_tables(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                          const double *theta12_host, double *S_B, double *L, int flags, int64_t *nan_counts,
                          fcd_stream stream);

/* ---- repeated sessions per patient: bt (C, U, K) -----------------------------------------------------------------
 * bt holds K >= 1 scans of every patient, contiguous with the session as the fastest index: bt[(c*U + u)*K + k].  F~_cu is
 * the patient's latent state of the connection and the sessions are conditionally independent measurements of it:
 *   P_j(c,u)  = prod_k N(bt[c,u,k]; mu_j, sigma_j)                (a NaN session contributes 1 with FCD_DATA_NAN_MISSING)
 *   M_kl(c,u) = e_l P_k + (1 - e_l)/2 sum_{j != k} P_j            (e_l = _eval_M_eps, as in fcd_lik_tables)
 * computed in log form, a_j = sum_k ln N_j (ascending k), m = max_j a_j, lM = m + ln M_kl(exp(a - m)): finite where the
 * product of the densities underflows.  An item with no observed session has lM = 0.0 exactly; a NaN session adds exactly
 * 0.0, so it leaves the other sessions' table bit for bit; m = -inf gives -inf.  Without the flag a NaN session makes its
 * item NaN.  Extra sessions of CONTROLS need nothing: they are extra columns of b.
 *
 * fcd_lik_tables_sessions: S_B (C,3) and lp_B_g_F (C,H,3; may be NULL) equal fcd_lik_tables_ex's bit for bit, lM (C,U,3,3)
 * as above; n_missing2 as in fcd_lik_tables_ex, its second word counting NaN session entries of bt.  There is no
 * p_Bt_g_Ft: the product of densities is what underflows.
 * fcd_lik_shared_tables_sessions: S_B and L (C,3,3), L[c] = sum_u lM[c,u] in fcd_lik_shared_tables' fixed order.
 * fcd_conn_posterior_sessions: fcd_conn_posterior_ex with the densities of an item taken over its sessions; an item with
 * no observed session gets the prior law of T and F~ given (k, l).
 * All three refuse K < 1 (FCD_ERR_ARG), K > INT32_MAX (FCD_ERR_UNSUPPORTED), unknown flags and what their siblings refuse.
 * Alignment: lM must be 16-byte aligned (ALIGNMENT, top of this file). */
int fcd_lik_tables_sessions(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U, int64_t K,
                            const double *theta12_host, double *S_B, double *lM, double *lp_B_g_F, int flags,
                            int64_t *n_missing2, fcd_stream stream);
int fcd_lik_shared_tables_sessions(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                   int64_t K, const double *theta12_host, double *S_B, double *L, int flags,
                                   int64_t *nan_counts, fcd_stream stream);
int fcd_conn_posterior_sessions(fcd_ctx *ctx, const double *bt, int64_t Nreg, int64_t U, int64_t K,
                                const double *theta12_host, const uint32_t *counts, const double *lq_F, const double *lq_R,
                                int flags, double *p_T, double *p_F_tilde, double *p_changed, fcd_stream stream);

/* ---- per-subject measurement noise: known sampling variances on top of the population spread --------------------------
 * Every control h and every session k of every patient u may carry a known variance v >= 0 (the sampling variance of its
 * correlations, e.g. from the number of frames kept):
 *   b_ch   | F_c = k   ~ N(mu_k, sigma_k^2 + var_b[h])
 *   bt_cuk | F~_cu = j ~ N(mu_j, sigma_j^2 + var_bt[u*K + k])      (sessions conditionally independent, as above)
 * sigma is then the population spread alone.  var_b is H doubles and var_bt U*K doubles (session fastest), both DEVICE
 * pointers; NULL means all zeros, and all zeros is the model of the sessions entry points.  bt is (C, U, K) as above, K = 1
 * for one scan per patient.  The tables are the sessions tables in log form with s_juk = sqrt(sigma_j^2 + var_bt[u,k]) in
 * place of sigma_j:  a_j = sum_k [-z^2/2 - (ln s_juk + ln sqrt(2 pi))], z = (x - mu_j)/s_juk, lM = m + ln M_kl(exp(a - m)).
 * A NaN entry adds exactly 0.0 under FCD_DATA_NAN_MISSING whatever its variance, an item with no observed session is 0.0,
 * m = -inf gives -inf; the NaN counts are those of the sessions entry points.  1/s and ln s + ln sqrt(2 pi) are made once
 * per call into a block the context owns (one small launch) and looked up per item: no division, square root or logarithm
 * per session.  Variances are not checked on the device: the caller passes finite values >= 0.
 *
 * fcd_lik_tables_noise: S_B (C,3), lM (C,U,3,3), lp_B_g_F (C,H,3; may be NULL).  With var_b NULL, S_B and lp_B_g_F equal
 * fcd_lik_tables_ex's bit for bit.
 * fcd_lik_shared_tables_noise: S_B and L (C,3,3) = sum_u lM[c,u]; the per-patient table is never written.
 * fcd_conn_posterior_noise: fcd_conn_posterior_sessions with the densities of these variances.
 * Refusals as the sessions entry points: K < 1 FCD_ERR_ARG, non-triangular C FCD_ERR_SHAPE, K > INT32_MAX or
 * U*K > 2^31 FCD_ERR_UNSUPPORTED, unknown flags FCD_ERR_ARG.
 * Alignment: lM must be 16-byte aligned (ALIGNMENT, top of this file). */
int fcd_lik_tables_noise(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U, int64_t K,
                         const double *theta12_host, const double *var_b, const double *var_bt, double *S_B, double *lM,
                         double *lp_B_g_F, int flags, int64_t *n_missing2, fcd_stream stream);
int fcd_lik_shared_tables_noise(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U, int64_t K,
                                const double *theta12_host, const double *var_b, const double *var_bt, double *S_B,
                                double *L, int flags, int64_t *nan_counts, fcd_stream stream);
int fcd_conn_posterior_noise(fcd_ctx *ctx, const double *bt, int64_t Nreg, int64_t U, int64_t K, const double *theta12_host,
                             const double *var_bt, const uint32_t *counts, const double *lq_F, const double *lq_R,
                             int flags, double *p_T, double *p_F_tilde, double *p_changed, fcd_stream stream);

/* ---- known groups of patients: one table per group ------------------------------------------------------------------
 * fcd_lik_grouped_tables: S_B (C,3) and L (C,G,3,3),
 *   L[c, g, k, l] = sum over the patients u of group g of lM[c, u, k, l],
 * the tables of the grouped-region model (one anomaly map per known group of patients): the collapsed joint of the unshared
 * model at G pseudo-patients.  Nothing of size C*U is written.  bt is (C, U, K) as in the sessions entry points, K = 1 for
 * one scan per patient.  var_b and var_bt both NULL select the sigma form (the terms of fcd_lik_shared_tables_sessions),
 * otherwise the record form of fcd_lik_shared_tables_noise with the variances given (a NULL one is all zeros); the record of
 * patient u is looked up with the gathered u.
 * order (U int32) lists the patients sorted by group and offsets (G + 1 int64) gives each group's span in it; both are
 * DEVICE pointers.  Every patient is in exactly one group and no group is empty: offsets[0] = 0, offsets[G] = U, strictly
 * increasing, order a permutation of 0 .. U-1.  The contents are the caller's to check on its host copy (fcdiff_amd.fit
 * .group_labels_csr makes and checks them); the call does not wait for the device to read them.  An order entry outside
 * [0, U) is skipped by the kernel, never dereferenced.
 * The sums have a fixed order (lane i of a group of 16, 32 or 64 lanes -- by the largest group, fcd_lik_shared_tables' rule --
 * takes members i, i + width, ... in `order`, then a butterfly), so two calls agree bit for bit; with one group L equals
 * fcd_lik_shared_tables_sessions' / _noise's bit for bit, with U singleton groups in patient order it equals
 * fcd_lik_tables_sessions' / _noise's lM.  S_B equals theirs bit for bit in every case.  nan_counts as in the shared entry
 * points (each patient is in one group, so each NaN is counted once).
 * Refusals: null pointers, unknown flags, K < 1, G < 1 or G > U FCD_ERR_ARG; non-triangular C FCD_ERR_SHAPE; K > INT32_MAX,
 * or U*K > 2^31 in the record form, FCD_ERR_UNSUPPORTED. */
int fcd_lik_grouped_tables(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U, int64_t K,
                           const double *theta12_host, const double *var_b, const double *var_bt, const int32_t *order,
                           const int64_t *offsets, int64_t G, double *S_B, double *L, int flags, int64_t *nan_counts,
                           fcd_stream stream);

/* ---- latent subtypes of patients: the two passes of the subtype-region model over the per-patient table ----------------
 * With responsibilities resp[u, g] = q(z_u = g), U patients and 1 <= G <= 8 subtypes, both fp64, both reading
 * lM (C, U, 3, 3) exactly once for all G, both with a fixed summation order and no atomics (two calls agree bit for bit).
 *
 * fcd_lik_weighted_tables: L (C, G, 3, 3),
 *   L[c, g, k, l] = sum_u resp[u, g] lM[c, u, k, l],
 * the table of the unshared model at G pseudo-patients that the variational updates of the subtype-region model run on
 * (fcd_lik_grouped_tables' L is the one-hot case).  A weight that is exactly 0 adds 0.0 whatever the entry, so 0 * -inf is 0;
 * with a positive weight -inf stays -inf.  resp is (U, G) row-major, a DEVICE pointer, not checked.  No workspace.
 *
 * fcd_vb_subtype_loglik: E (U, G),
 *   E[u, g] = sum_c sum_k q_F[c,k] sum_l w_l^g(c) lM[c, u, k, l]
 * with lq_F (C, 1, 3), lq_R (Nreg, G, 2) the subtypes' q_R and w^g(c) its mixture-case weights at the true endpoints of c, in
 * the case order and with the products of fcd_vb_patient_elbo's E_lM term (q * lM is a plain product).  E[u, :] does not
 * depend on the other patients of the call.  Uses the context's workspace.
 *
 * Refusals: null pointers, G < 1 or G > 8, U < 1, L aliasing lM FCD_ERR_ARG; a non-triangular C or Nreg < 2 FCD_ERR_SHAPE;
 * Nreg > 46340, U > 2^24 or more than 2^31 - 1 workgroups FCD_ERR_UNSUPPORTED. */
int fcd_lik_weighted_tables(fcd_ctx *ctx, const double *lM, const double *resp, int64_t C, int64_t U, int64_t G, double *L,
                            fcd_stream stream);
int fcd_vb_subtype_loglik(fcd_ctx *ctx, const double *lq_F, const double *lq_R, const double *lM, int64_t Nreg, int64_t U,
                          int64_t G, double *E, fcd_stream stream);

/* ---- forward sampler: UnsharedRegionModel.sample, fcdiff/model.py:52-236, on the device ---------------
 * Counter RNG (Philox), all variables drawn in parallel; the reference's MT19937 stream is not reproduced (the host
 * sampler of the Python mirror does that) -- same distribution.  Type INDICES are returned: r (Nreg,U), t (C,U),
 * f (C,), f_tilde (C,U) uint8; b (C,H), b_tilde (C,U) float64 clipped to [-1,1].  Edges in the fitter's order. */
int fcd_model_sample(fcd_ctx *ctx, const double *theta12_host, int64_t Nreg, int64_t H, int64_t U, uint64_t seed, uint8_t *r,
                     uint8_t *t, uint8_t *f, uint8_t *f_tilde, double *b, double *b_tilde, fcd_stream stream);
/* The same for the shared-region model (SharedRegionModel): r (Nreg,) is drawn once per region and holds for every
 * patient; t, f_tilde and b_tilde of each patient read it.  Other outputs as fcd_model_sample. */
int fcd_model_sample_shared(fcd_ctx *ctx, const double *theta12_host, int64_t Nreg, int64_t H, int64_t U, uint64_t seed,
                            uint8_t *r, uint8_t *t, uint8_t *f, uint8_t *f_tilde, double *b, double *b_tilde,
                            fcd_stream stream);

/* ---- front-end: region x time series -> edge-major correlations --------------------------------------
 * Not in the reference (its inputs are already correlations, fit.py:20-23); oracle = numpy.corrcoef.
 * ts (S, Nreg, T) -> out (C, S), out[c][s] = corrcoef(ts[s])[n, m] for c = n(n-1)/2 + m, n > m: the layout of
 * b / bt.  fp64 MFMA Gram product per subject.  fisher_z != 0 applies atanh; keep it 0 with the reference's model
 * defaults, which are calibrated on raw correlations clipped to [-1, 1] (fcdiff/model.py:213, 236).
 * Alignment: ts must be 16-byte aligned when T is even (ALIGNMENT, top of this file). */
int fcd_corr_edges(fcd_ctx *ctx, const double *ts, int64_t S, int64_t Nreg, int64_t T, int fisher_z, double *out,
                   fcd_stream stream);
/* Cleaning in front of it: frame censoring and confound regression, per subject and over its kept frames only.
 * ts (S, Nreg, T); confounds (S, Q, T), 0 <= Q <= 64, NULL allowed when Q == 0 (an intercept is always implied);
 * frame_mask (S, T) bytes, non-zero keeps the frame, NULL keeps all.  A dropped frame is never read into a sum: NaN or
 * inf stored there does not reach the result.  Rows are centred over the kept frames; constant confounds are dropped,
 * the others scaled to unit norm and collinear ones dropped by pivoted Cholesky of their Gram matrix (remaining squared
 * norm below 1e-10); resid = y_c - beta^T x_c from the normal equations of the columns used.
 * resid (S, Nreg, T), caller-owned: the residuals of the kept frames in order at positions 0 .. n_kept - 1, exact zeros
 * behind them.  A row is all zeros (its edges then come out NaN) when it is constant or holds a non-finite value over
 * the kept frames, when its residual sum of squares is <= 1e-20 of its centred sum of squares, or when its subject has
 * dof < 2 or a non-finite kept value in a confound (rank is then reported as 0).
 * info (S, 3) int32, caller-owned: n_kept, rank (confound columns used), dof = n_kept - 1 - rank.
 * The call sequence fcd_corr_clean; fcd_corr_edges(resid) gives the correlations of the residuals: zero-mean rows
 * followed by zeros have the same correlation over T frames as over n_kept.  Deterministic; inputs are not written. */
int fcd_corr_clean(fcd_ctx *ctx, const double *ts, const double *confounds, const uint8_t *frame_mask, int64_t S,
                   int64_t Nreg, int64_t Q, int64_t T, double *resid, int32_t *info, fcd_stream stream);
/* Partial correlations with shrinkage towards the identity, per subject; oracle = tests/partial_corr_ref.py.
 * ts (S, Nreg, T), 2 <= Nreg <= 1024; n_frames (S,) int32 or NULL (= T): subject s counts its first n = n_frames[s] frames.
 * With n < T the rows must be what fcd_corr_clean leaves -- zero mean over the first n frames, exact zeros behind them
 * (pass its info[:, 0]); the padding then enters no sum.
 *   1  A region is dead for the subject where fcd_corr_edges gives NaN on all of its edges (a constant or all-zero row, a
 *      non-finite value).  Dead regions leave the problem: p = the number of live ones, all their edges come out NaN, and
 *      the inverse below is that of the live p x p block.
 *   2  R = the sample correlation matrix of the live rows (its off-diagonals are fcd_corr_edges' values).
 *   3  R_a = (1 - a) R + a I.  shrink_mode 0: a = shrink_value in [0, 1].  shrink_mode 1: Ledoit & Wolf (2004) on the
 *      standardised rows z_it = (x_it - m_i) / s_i, s_i^2 = sum_t (x_it - m_i)^2 / n:  q_t = sum_i z_it^2, B = sum_t q_t^2,
 *      F = p + 2 sum_{i>j} R_ij^2, beta = (B / n - F) / (p n), delta = (F - p) / p, a = 0 if delta <= 0 or beta <= 0, else
 *      min(beta, delta) / delta.
 *   4  Theta = R_a^-1 by blocked Gauss-Jordan without pivoting.  A pivot <= 1e-12 (a = 0 with n - 1 < p, duplicate rows):
 *      the subject is numerically singular, all of its edges are NaN and its status says so; nothing is regularised.
 *   5  out[c][s] = -Theta_nm / sqrt(Theta_nn Theta_mm) clipped to [-1, 1], c = n(n-1)/2 + m (n > m); fisher_z != 0: atanh.
 * out (C, S); alpha (S,): the a used (NaN where status is 2 or 3); info (S, 2) int32: p_live, status -- 0 ok, 1 singular,
 * 2 p_live < 2, 3 n_frames[s] outside [0, T] (checked on the device); every status but 0 leaves the subject's column NaN.
 * The correlations are made by fcd_corr_edges' kernels; subjects are walked in chunks whose dense matrices stay below
 * 256 MB (knob "partial_chunk": at most so many subjects per chunk), which changes no bit.  Uses the context's workspace.
 * Deterministic (fixed reduction orders, no floating-point atomics); inputs are not written.
 * FCD_ERR_ARG: null pointer, S, Nreg or T < 1, shrink_value outside [0, 1] or NaN in mode 0.  FCD_ERR_UNSUPPORTED: Nreg > 1024,
 * unknown shrink_mode, S > 65535.  FCD_ERR_SHAPE: Nreg < 2 or T < 2, as fcd_corr_edges.
 * Alignment: ts must be 16-byte aligned when T is even (ALIGNMENT, top of this file). */
int fcd_corr_partial(fcd_ctx *ctx, const double *ts, int64_t S, int64_t Nreg, int64_t T, const int32_t *n_frames,
                     int shrink_mode, double shrink_value, int fisher_z, double *out, double *alpha, int32_t *info,
                     fcd_stream stream);

/* ---- covariate adjustment of the connections, fitted on the controls -----------------------------------------------------
 * Not in the reference; oracle = tests/covariates_ref.py.  For every connection c, ordinary least squares with an implied
 * intercept over the controls observed at c:  b[c,h] = alpha_c + sum_q beta[c,q] z[h,q] + e.
 * b (C, H) and z (H, Q) fp64, 0 <= Q <= 16 (z and beta may be NULL when Q == 0); C need not be triangular.  z is finite (not
 * checked here).  flags: FCD_DATA_NAN_MISSING -- a NaN b[c,h] leaves control h out of connection c's fit; without it every
 * control counts (n_obs = H) and a NaN makes that row of beta, and its resid_var, NaN.
 * The rules of fcd_corr_clean: columns are centred over the connection's observed controls; a column constant over them
 * (min == max) is dropped; the others are scaled to unit norm (remaining squared norm exactly 1 before the first pivot);
 * collinear columns are dropped by diagonally pivoted Cholesky of the Gram matrix (remaining squared norm below 1e-10, ties
 * to the lowest column index); beta from the normal equations of the columns used.
 * beta (C, Q): in the units of the columns of z, 0 for a column not used.  resid_var (C,): sum of squared residuals / dof,
 * from the residuals themselves.  info (C, 4) int32: n_obs, rank (columns used), dof = n_obs - 1 - rank, bit mask of the
 * columns used.  A connection with dof < 1 is not fitted: beta row 0, rank and mask reported as 0 (dof as found), resid_var
 * NaN.  Any H: the design is walked four controls at a time and never held whole on chip.  Two launches; uses the context's
 * workspace (2 x H x 16 doubles + 144 bytes): fcd_ctx_reserve knows nothing of H and does not size it, so a call with H > 4095
 * (more than the workspace's first megabyte) grows it once, as any call with a larger shape than before does.
 * Deterministic; inputs are not written.
 * FCD_ERR_UNSUPPORTED for Q > 16, unknown flags or H > 2^26; FCD_ERR_ARG for C < 1, H < 1, Q < 0 or a null pointer. */
int fcd_edge_cov_fit(fcd_ctx *ctx, const double *b, int64_t C, int64_t H, const double *z, int64_t Q, int flags, double *beta,
                     double *resid_var, int32_t *info, fcd_stream stream);
/* out[c,s] = x[c,s] - d,  d = sum_q beta[c,q] (z[s,q] - z_ref[q]) added up over q ascending from 0.0, one rounded product and
 * one rounded sum per term: a NumPy loop's result bit for bit.  x, out (C, S), z (S, Q), z_ref (Q,), beta (C, Q),
 * all device.  NaN stays NaN.  Sessions are the caller's flattening of (U, K) to S.  One launch.  Refusals as above.
 * Alignment: the path is chosen by the address -- x and out both 16-byte aligned and S even take the 16-byte path,
 * anything else the 8-byte one, with the same bits (ALIGNMENT, top of this file). */
int fcd_edge_cov_apply(fcd_ctx *ctx, const double *x, int64_t C, int64_t S, const double *z, int64_t Q, const double *z_ref,
                       const double *beta, double *out, fcd_stream stream);

/* ---- site harmonisation (ComBat) fitted on the controls ---------------------------------------------------------------------
 * Not in the reference; oracle = tests/harmonize_ref.py.  Location and scale per site and connection, shrunk by empirical
 * Bayes towards the site's law over all connections (Johnson et al. 2007), the site parameters fitted on the controls alone
 * and then applied to anybody.  Both entry points take one descriptor; a member an entry point does not name is not read.
 *
 * Fit, per connection c over the controls observed there (FCD_DATA_NAN_MISSING: a NaN b[c,h] is unobserved and adds 0;
 * without it every control counts and a NaN makes the connection "not fitted"), i(h) = site[h], n_i observed at site i,
 * n = sum n_i, B_c = sites with n_i >= 1:
 *   1  ybar_i = mean of site i;  d = W^T y;  e_h = (y_h - ybar_i(h)) - sum_q d_q W[h,q];  beta = T d;
 *      sigma2 = sum_h e_h^2 / n (divided by n, not by the degrees of freedom), from the residuals themselves;
 *   2  alpha_i = ybar_i - (z_bar_i - z_ref) . beta;  abar = sum_i (n_i / n) alpha_i;  gamma_hat_i = (alpha_i - abar) / sigma
 *      where n_i >= 1;  delta2_hat_i = sum_{h in i} e_h^2 / (sigma2 (n_i - 1)) where n_i >= 2;  NaN where they do not exist;
 *   3  status (info[c][3]): 0 fitted; 1 n - B_c - Qp < 1; 2 sum e^2 == 0; 3 a NaN that is not missing data; 4 a site id
 *      outside 0..B-1 among the H (every connection; the context's error word is set too: fcd_ctx_check,
 *      fcd_ctx_clear_error).  Not fitted: grand_mean, pooled_sd, the row of beta and the gamma / delta2 columns are NaN,
 *      shift 0, scale 1, n_iter 0, and the connection enters no prior;
 *   4  per site over the fitted connections where the estimate exists: gamma_bar, tau2 = mean and variance (ddof 1) of
 *      gamma_hat_i, m, s2 those of delta2_hat_i, each in two passes (mean, then centred squares), a = (2 s2 + m^2) / s2,
 *      b = (m s2 + m^3) / s2.  Undefined (prior_info[i][2] == 0, a and b NaN) with fewer than two members in either set or
 *      where tau2 or s2 is not > 0 and finite: the site's pairs are then left alone (stars NaN, shift 0, scale 1);
 *   5  per (site, fitted connection) the fixed point of  gamma <- (n_i tau2 gamma_hat + delta2 gamma_bar) / (n_i tau2 + delta2),
 *      delta2 <- (((n_i - 1) delta2_hat + n_i (gamma_hat - gamma)^2) / 2 + b) / (n_i / 2 + a - 1)  from (gamma_hat, delta2_hat),
 *      until |step of gamma| <= 1e-13 (1 + |gamma|) and |step of delta2| <= 1e-13 delta2, at most 1000 steps; n_iter is the
 *      number of steps, NEGATIVE where the cap was hit.  n_i == 1: (n_i - 1) delta2_hat is 0 and delta2 starts at b / (a - 1);
 *      n_i == 0: the prior, gamma_bar and b / (a - 1), 0 steps.  (ComBat stops all connections jointly at 1e-4: the same
 *      fixed point, solved tightly.)  FCD_HARMONIZE_NO_EB: the stars are the hats, no prior is made (all NaN, counts 0), and
 *      a pair with n_i < 2 or delta2_hat == 0 is left alone (shift 0, scale 1);
 *   6  shift = sigma gamma_star, scale = sqrt(delta2_star).
 * Apply, for subject s at site[s] with covariates z[s]:  d = sum_q beta[c,q] (z[s,q] - z_ref[q]) over q ascending from 0.0,
 * m = grand_mean[c] + d,  out = ((x - m) - shift) / scale + m, one rounded operation per step in this order; NaN stays NaN.
 * A pair with shift == 0 and scale == 1 is copied: out has x's bits.  A site id outside 0..B-1 gives NaN and sets the
 * context's error word.
 * Three launches for the fit (plus one per 128 doubles of T and of z_bar), one for apply; the fit uses 4.6 KB of the context's
 * workspace.  Deterministic (fixed summation orders, no floating-point atomics); inputs are not written.
 * FCD_ERR_ARG: null context, descriptor or needed pointer, size != sizeof(fcd_harmonize_desc), C, B, H (fit) or S (apply)
 * < 1, Q < 0, Qp outside 0..Q.  FCD_ERR_UNSUPPORTED: unknown flags, B > 64, Q > 8, H > 4096, Qp > 0 together with
 * FCD_DATA_NAN_MISSING (every connection would need a design of its own). */
#define FCD_HARMONIZE_NO_EB 2
typedef struct fcd_harmonize_desc {
    uint32_t size;             /* sizeof(fcd_harmonize_desc): the version of the layout */
    uint32_t flags;            /* FCD_DATA_NAN_MISSING | FCD_HARMONIZE_NO_EB (fit) */
    int64_t C;                 /* connections (need not be triangular) */
    int64_t H;                 /* fit: controls, <= 4096 */
    int64_t S;                 /* apply: subjects (sessions flattened by the caller) */
    int64_t B;                 /* sites, <= 64 */
    int64_t Q;                 /* covariate columns, <= 8 */
    int64_t Qp;                /* fit: columns of the design that are used, <= Q */
    fcd_stream stream;         /* every launch goes here */
    /* device, read */
    const double *b;           /* fit: (C, H) */
    const uint8_t *site;       /* fit: (H,), apply: (S,); values 0..B-1 */
    const double *W;           /* fit: (H, Qp) orthonormal basis of the used columns, each centred within every site */
    const double *x;           /* apply: (C, S) */
    const double *z;           /* apply: (S, Q) */
    /* host, read before the call returns (NULL where Q == 0) */
    const double *T;           /* fit: (Q, Qp), beta = T (W^T y) in the units of the original columns */
    const double *z_bar;       /* fit: (B, Q) the sites' means of the covariates */
    const double *z_ref;       /* both: (Q,) the point the harmonised values refer to */
    /* device, written by the fit; apply reads grand_mean, beta, shift and scale */
    double *grand_mean;        /* (C,) abar */
    double *pooled_sd;         /* (C,) sigma */
    double *beta;              /* (C, Q) */
    double *gamma_hat;         /* (B, C), as the five planes below */
    double *delta2_hat;
    double *gamma_star;
    double *delta2_star;
    double *shift;
    double *scale;
    int32_t *n_obs;            /* (B, C) n_i */
    int32_t *n_iter;           /* (B, C) */
    int32_t *info;             /* (C, 4) n, B_c, Qp, status */
    double *prior;             /* (6, B) gamma_bar, tau2, m, s2, a, b */
    int32_t *prior_info;       /* (B, 3) members of the gamma set, of the delta2 set, 1 where the prior is defined */
    /* device, written by apply */
    double *out;               /* (C, S) */
} fcd_harmonize_desc;
int fcd_site_harmonize_fit(fcd_ctx *ctx, const fcd_harmonize_desc *d);
/* fcd_site_harmonize_apply: Alignment: the path is chosen by the address -- x and out both 16-byte aligned and S even take the 16-byte path,
 * anything else the 8-byte one, with the same bits (ALIGNMENT, top of this file). */
int fcd_site_harmonize_apply(fcd_ctx *ctx, const fcd_harmonize_desc *d);

/* ---- batched symmetric eigendecomposition -------------------------------------------------------------------------------------
 * A (B, n, n) fp64, device, symmetric (only the lower triangle is read), not necessarily definite; 1 <= n <= 1024.
 * w (B, n): the eigenvalues ascending; V (B, n, n): column k of V[b] is the unit eigenvector of w[b][k]; status (B,) int32:
 * 0 ok, 1 a non-finite entry (or entries whose squares overflow), 2 not converged; w and V of a matrix whose status is not 0
 * are NaN, and it changes nothing of its neighbours in the batch.
 * Two-sided parallel cyclic Jacobi, one workgroup per matrix: round-robin pairing (a bye for odd n), an off-diagonal at or
 * below 2^-58 ||A||_F is not rotated, a sweep without a rotation ends the loop, 40 sweeps at the most.  A diagonal matrix is
 * therefore returned as it is (sorted), exactly.  Up to n = 96 the matrix and the eigenvectors stay in LDS; above, they live in
 * the context's workspace (2 n^2 doubles per matrix of a chunk of at most 512 MB, or of at most "tangent_chunk" matrices where
 * that knob is > 0; successive chunks reuse it, and the chunking changes no bit).  Deterministic; A is not written.
 * FCD_ERR_ARG: null context, descriptor or pointer, size != sizeof(fcd_eigh_desc), B or n < 1.  FCD_ERR_UNSUPPORTED: n > 1024,
 * B > 2^24, flags != 0. */
typedef struct fcd_eigh_desc {
    uint32_t size;             /* sizeof(fcd_eigh_desc): the version of the layout */
    uint32_t flags;            /* 0 */
    int64_t B;                 /* matrices */
    int64_t n;                 /* their order, <= 1024 */
    fcd_stream stream;         /* every launch goes here */
    const double *A;           /* device, read: (B, n, n) */
    double *w;                 /* device, written: (B, n) */
    double *V;                 /* (B, n, n) */
    int32_t *status;           /* (B,) */
} fcd_eigh_desc;
int fcd_sym_eigh(fcd_ctx *ctx, const fcd_eigh_desc *d);

/* ---- tangent-space connectivity fitted on the controls ----------------------------------------------------------------------
 * Not in the reference; oracle = tests/tangent_ref.py (Varoquaux et al. 2010; kind="tangent" of nilearn, on correlation
 * matrices).  Both entry points take one descriptor; a member an entry point does not name is not read.
 *
 * Per subject s, over its first n = n_frames[s] frames (NULL: T; rows as fcd_corr_partial wants them):
 *   1  live regions, R, alpha and R_a = (1 - a) R + a I exactly as rules 1 - 3 of fcd_corr_partial (the same kernels).  The
 *      correlation matrix is shrunk, not the covariance: the result does not depend on the scale of a region's series.
 *   2  A matrix function acts on the whole matrix, so a dead region cannot leave the problem for one subject only: a subject
 *      with 2 <= p_live < Nreg has status 4 and is all NaN.  The remedy is the caller's: drop that region for everyone.
 *   3  status (info[s][1]): 0 ok; 1 numerically singular -- the fit asks lambda_min(R_a) <= 1e-12 lambda_max(R_a) of every
 *      control, apply asks the same of M_s = W R_a W, which has R_a's inertia (a = 0 with n - 1 < p, duplicate rows); 2
 *      p_live < 2; 3 n_frames[s] outside [0, T]; 4 a dead region; 5 the eigensolver gave up on a matrix of this subject (a
 *      non-finite entry, as a non-finite W makes them, or no convergence).  Every status but 0 leaves the subject NaN;
 *      nothing is regularised.  alpha is NaN for 2 and 3, as fcd_corr_partial's.
 * Fit (ts = the controls, S of them):
 *   4  used[s] = 1 where status is 0.  Fewer than two used controls: FCD_ERR_ARG.
 *   5  G = the arithmetic mean of the used R_a, added in the order of the controls.  FCD_TANGENT_EUCLIDEAN: that is the
 *      reference.  Otherwise the Frechet mean of the affine-invariant metric by the fixed point, from that G:
 *         W = G^-1/2;  Tbar = mean over the used controls, in their order, of logm(W R_a,s W);
 *         stop if ||Tbar||_F <= tol sqrt(Nreg) (converged) or after max_iter evaluations of Tbar (not converged);
 *         G <- G^1/2 expm(Tbar) G^1/2
 *      *n_iter = the number of evaluations of Tbar, NEGATIVE where the cap was hit; *grad_norm = the last ||Tbar||_F (NaN for
 *      the Euclidean reference); G, G_half and W always belong to one and the same G.  A G with an eigenvalue <= 1e-12 of its
 *      largest, or whose decomposition fails: FCD_ERR_ARG after the outputs are written.
 *   6  The fit synchronises the stream once to count the used controls and once per iteration to read the norm.
 * Apply (ts = any subjects; W = G^-1/2 (Nreg, Nreg), symmetric, from a fit or from the caller):
 *   7  T_s = logm(W R_a,s W): M_s = W R_a W (the lower tiles computed and mirrored), M_s = V L V^T by fcd_sym_eigh's kernel,
 *      T_s = V log(L) V^T (lower tiles, mirrored).  out[c][s] = T_s[n][m], c = n(n-1)/2 + m (n > m), unscaled (no sqrt 2);
 *      diag[i][s] = T_s[i][i].  Never synchronises.  W lies on the device and is not looked at by the host: a non-finite W
 *      gives every subject status 5.
 * Subjects are walked in chunks whose matrices stay below 128 MB each (knob "tangent_chunk"); the mean over the controls is a
 * running sum in their order, so the chunking changes no bit, and a subject alone gives the bits it has inside a batch.
 * Deterministic (fixed reduction orders, no floating-point atomics); inputs are not written.  Uses the context's workspace;
 * the fit keeps the R_a of all controls there (S x PL^2 doubles, PL = 16 ceil(Nreg / 16)).
 * FCD_ERR_ARG: null context, descriptor or needed pointer, size != sizeof(fcd_tangent_desc), S, Nreg or T < 1, shrink_value
 * outside [0, 1] or NaN in mode 0, tol not > 0 or max_iter < 1 for the geometric fit.  FCD_ERR_UNSUPPORTED: unknown flags or
 * shrink_mode, Nreg > 1024, S > 65535, a fit above 64 GiB of workspace.  FCD_ERR_SHAPE: Nreg < 2 or T < 2. */
#define FCD_TANGENT_EUCLIDEAN 1
typedef struct fcd_tangent_desc {
    uint32_t size;             /* sizeof(fcd_tangent_desc): the version of the layout */
    uint32_t flags;            /* fit: FCD_TANGENT_EUCLIDEAN */
    int64_t S;                 /* subjects (fit: controls), <= 65535 */
    int64_t Nreg;              /* 2 .. 1024 */
    int64_t T;                 /* frames */
    int32_t shrink_mode;       /* 0: alpha = shrink_value; 1: Ledoit-Wolf per subject */
    int32_t max_iter;          /* fit, geometric: >= 1 */
    double shrink_value;
    double tol;                /* fit, geometric: > 0 */
    fcd_stream stream;         /* every launch goes here */
    /* device, read */
    const double *ts;          /* (S, Nreg, T) */
    const int32_t *n_frames;   /* (S,) or NULL */
    /* device, written by both */
    double *alpha;             /* (S,) */
    int32_t *info;             /* (S, 2) p_live, status */
    /* device, written by the fit; apply reads W */
    double *G;                 /* (Nreg, Nreg) */
    double *G_half;            /* (Nreg, Nreg) G^1/2 */
    double *W;                 /* (Nreg, Nreg) G^-1/2 */
    uint8_t *used;             /* (S,) */
    /* host, written by the fit */
    int32_t *n_iter;
    double *grad_norm;
    /* device, written by apply */
    double *out;               /* (C, S) */
    double *diag;              /* (Nreg, S) */
} fcd_tangent_desc;
/* fcd_tangent_fit: Alignment: ts must be 16-byte aligned when T is even (ALIGNMENT, top of this file). */
int fcd_tangent_fit(fcd_ctx *ctx, const fcd_tangent_desc *d);
/* fcd_tangent_apply: Alignment: ts must be 16-byte aligned when T is even (ALIGNMENT, top of this file). */
int fcd_tangent_apply(fcd_ctx *ctx, const fcd_tangent_desc *d);

/* ---- classical baselines ---------------------------------------------------------------------------------------------------
 * Not in the reference; oracle = tests/baseline_ref.py.  b (C, H) controls, bt (C, U) patients, fp64, device; C triangular,
 * connections in the order of fcd_c_to_nm.  E(n) = the Nreg - 1 connections that touch region n.  Both calls are deterministic
 * (fixed reduction orders, integer atomics only) and write no input.
 *
 * Normative scores.  Per connection over the controls observed there (a NaN is unobserved): n_c, mean m_c, s_c^2 = sum
 * (x - m_c)^2 / (n_c - 1) in two passes.  z[c,u] = (bt[c,u] - m_c) / (s_c sqrt(1 + 1/n_c)); the leave-one-out score of control h,
 * z0[c,h], is the same with mean and deviation of the OTHER n_c - 1 observed controls, their sums taken directly (no
 * downdate), and n_c - 1 for n_c.  A score is NaN where n_c < 3, where the deviation is not > 0, or where the value is NaN.
 * Per region n and subject: n_edges = defined scores over E(n), msq = mean of z^2 over them (NaN if none), n_over = those
 * with |z| > z_threshold.  msq0, n_edges0, n_over0 (Nreg, H) and msq, n_edges, n_over (Nreg, U); n_controls (C,) = n_c;
 * z0 (C, H) and z (C, U) may be NULL (not written).  One launch, no workspace.
 * FCD_ERR_SHAPE for a non-triangular C; FCD_ERR_UNSUPPORTED for H > 1024 (a control row lives in LDS) or
 * H + U > 65535 * 64; FCD_ERR_ARG for a null pointer or a size < 1. */
int fcd_baseline_normative(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U, double z_threshold,
                           double *msq0, int32_t *n_edges0, int32_t *n_over0, double *msq, int32_t *n_edges, int32_t *n_over,
                           int32_t *n_controls, double *z0, double *z, fcd_stream stream);
/* Two-sample permutation test.  X = [b | bt] (C, S), S = H + U, complete (NaN is not checked here and spreads), rows centred on
 * their mean over S, Q_c = sum x^2.  For a labelling l in {0,1}^S with U ones: A = sum l_s x_s, g = A^2 S/(U H),
 * t^2 = g (S - 2) / (Q_c - g) -- the square of Student's pooled-variance t -- t = sign(A) sqrt(t^2), R[n] = sum over E(n) of t^2.
 * labels (P, S) bytes, non-zero = 1 (that a row has U ones is the caller's to check).  The observed labelling has its ones on
 * the last U subjects; it runs through the same tile product, the same t^2 and the same order of sums as the permutations,
 * so a row of labels equal to it gives its statistics bit for bit.
 * t (C,), region (Nreg,): observed.  null_max_t (P,) = max_c |t|, null_max_region (P,) = max_n R.  count_t (C,) = number of
 * rows with t^2 >= the observed t^2, count_region (Nreg,) = rows with R >= the observed R.
 * A constant connection (all S values equal) has centred values and Q of exactly 0: t = NaN, exactly 0 to every R, no part in
 * a maximum, count_t = 0, never a set bit below.  Where Q_c - g, a difference of two rounded numbers, is not > 0 with Q_c > 0,
 * t^2 = +inf and t = +/-inf with the sign of A; inf >= inf counts.  No other finite input gives a NaN.  No (P, C) array exists anywhere:
 * the sums A are an fp64 MFMA product whose tiles are reduced in registers.  Seven launches; uses the context's workspace
 * (about 8 C S + 16 Nreg P bytes), grown on demand.
 * FCD_ERR_SHAPE for a non-triangular C; FCD_ERR_UNSUPPORTED for S > 1024 (the labels of a permutation are 8 words per lane)
 * or P > 65535 * 128; FCD_ERR_ARG for a null pointer, a size < 1 or S < 3. */
int fcd_baseline_group_perm(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                            const uint8_t *labels, int64_t P, double *t, double *region, double *null_max_t,
                            double *null_max_region, int64_t *count_t, int64_t *count_region, fcd_stream stream);
/* Network-based statistic (Zalesky et al. 2010), in two halves.
 * The bits: the t^2 of the permutation test above (same centring, same tile product, same formula), each connection once,
 * kept as ONE BIT per (labelling, connection): set where t^2 > threshold^2 and, for FCD_TAIL_GREATER / _LESS, the sum A over
 * the labelled subjects is > 0 / < 0 (patients above / below controls).  bits (P, W) uint32, W = ceil(C / 32): bit c & 31 of
 * word c >> 5; the bits behind C in the last word are written as 0.  labels (P, S) bytes as above, or NULL with P = 1: the
 * observed labelling, which goes through the same kernel, so a row of labels equal to it gives its bits exactly.
 * t (C,), nullable: the signed t of labelling 0 (what the observed call is asked for).  No (P, C) array of doubles exists.
 * Three launches; workspace about 8 C S bytes.
 * FCD_ERR_SHAPE for a non-triangular C; FCD_ERR_UNSUPPORTED for more than 1024 regions, S > 1024 or P > 65535 * 64;
 * FCD_ERR_ARG for a null pointer, a size < 1, S < 3, labels == NULL with P != 1, a threshold that is not finite and > 0, or
 * an unknown tail. */
#define FCD_TAIL_BOTH 0
#define FCD_TAIL_GREATER 1
#define FCD_TAIL_LESS 2
int fcd_baseline_network_bits(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                              const uint8_t *labels, int64_t P, double threshold, int tail, uint32_t *bits, double *t,
                              fcd_stream stream);
/* The two calls above with options, flags = FCD_BASELINE_MISSING | FCD_BASELINE_WELCH; flags = 0 is the call above itself.
 * FCD_BASELINE_MISSING: a NaN in b or bt is an unobserved value (an infinite value is not checked here and spreads).  Per
 * connection c: O = the subjects observed there, n = |O|; the row is centred on its mean over O, x_s = 0 for a missing
 * subject, Q = sum x^2; the connection is constant where all observed values are equal (x and Q exactly 0).  Per labelling l
 * (still U ones over all S subjects, observed or not): n1 = sum over O of l_s, n0 = n - n1, A = sum l_s x_s, B = sum l_s x_s^2,
 * k = n / (n1 n0); the mean difference is A k.  Without the flag n = S and n1 = U.
 *   pooled (no FCD_BASELINE_WELCH)  defined iff the connection is not constant, n >= 3, n1 >= 1 and n0 >= 1.  g = A^2 k,
 *       t^2 = g (n - 2) / (Q - g), +inf where Q - g is not > 0; on complete data the call above operation for operation.
 *   FCD_BASELINE_WELCH  defined iff the connection is not constant, n1 >= 2 and n0 >= 2.  SS1 = max(B - A^2/n1, 0),
 *       SS0 = max((Q - B) - A^2/n0, 0), v = SS1/(n1 (n1 - 1)) + SS0/(n0 (n0 - 1)), t^2 = (A k)^2 / v; where v is not > 0,
 *       t^2 = +inf if A != 0 and 0 if A = 0.
 * The sign of t is that of A.  A value that is undefined under a labelling adds exactly 0 to every region sum, enters no
 * maximum and is never a set bit, but counts as an exceedance in count_t (a labelling that cannot be evaluated never makes a
 * p-value smaller).  A connection that is undefined under the observed labelling is dead, as a constant one: t = NaN,
 * count_t = 0, no part in region or in any permuted sum, maximum or bit.  A row of labels equal to the observed labelling
 * still gives the observed statistics bit for bit.  n_controls, n_patients (C,), each nullable: the observed controls and
 * patients per connection (H and U without FCD_BASELINE_MISSING).  The accumulators n1 and B go through the same fp64 MFMA tile
 * product as A; the observation mask travels as bits (nw C 16 bytes of workspace more, nw = ceil(S / 128)).
 * Refusals as for the calls above; other bits in flags FCD_ERR_UNSUPPORTED; FCD_BASELINE_WELCH with H < 2 or U < 2
 * FCD_ERR_ARG; fcd_baseline_network_bits_opt takes P <= 65535 * 32 with a flag set. */
#define FCD_BASELINE_MISSING 1
#define FCD_BASELINE_WELCH 2
int fcd_baseline_group_perm_opt(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                const uint8_t *labels, int64_t P, int flags, double *t, double *region, double *null_max_t,
                                double *null_max_region, int64_t *count_t, int64_t *count_region, int64_t *n_controls,
                                int64_t *n_patients, fcd_stream stream);
/* The bits with the same options and rules: a value undefined under its labelling, and every value of a connection that is
 * undefined under the observed labelling, is never a set bit; t (labelling 0) is NaN there. */
int fcd_baseline_network_bits_opt(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                  const uint8_t *labels, int64_t P, double threshold, int tail, int flags, uint32_t *bits,
                                  double *t, fcd_stream stream);
/* The two calls with nuisance covariates: the permutation GLM of Freedman & Lane (1983).  design (S, R) fp64, row-major, on the
 * device: its columns are orthonormal and each is orthogonal to the constant vector (the caller's to make so; fcdiff_amd's
 * baseline.glm_design does); column 0 is the contrast, tested given columns 1 .. R - 1.  The library does not know where the
 * design came from: any regressor, residualised on the others and the constant and scaled to unit norm, can stand in column 0.
 * Per connection e = the row minus its mean minus sum_{q >= 1} w_q (w_q^T row), Q_e = sum e^2.  perms (P, S) uint16, each row
 * a permutation of 0 .. S - 1 (the caller's to check; an index > S - 1 is read as a row of zeros): subject s gets design row
 * perms[p][s].  d_q = sum_s design[perms[p][s]][q] e_s, t^2 = d_0^2 dof / (Q_e - sum_q d_q^2) with dof = S - R - 1,
 * t = sign(d_0) sqrt(t^2), R[n] = sum over E(n) of t^2.  The observed statistics are those of the identity, run through the same
 * tile product, the same t^2 and the same order of sums, so a row of perms equal to the identity gives them bit for bit.
 * Outputs and rules as for fcd_baseline_group_perm: a constant connection is dead (t = NaN, 0 to every R, no maximum,
 * count_t = 0, never a set bit); where the denominator is not > 0 with the connection alive, t^2 = +inf with the sign of d_0.
 * Dead too: a connection with Q_e <= (8 S R 2^-52)^2 Q_c, Q_c the centred sum of squares of the row -- a linear function of the
 * covariates to rounding.  The d_q are an fp64 MFMA product whose A operand is read from the design in LDS by the permuted
 * index; no (P, C) array exists.  Seven launches; workspace about 8 C S + 16 Nreg P + P S / 2 bytes.
 * FCD_ERR_SHAPE for a non-triangular C; FCD_ERR_UNSUPPORTED for R < 1, R > 9, S > 1024 or P > 65535 * 128; FCD_ERR_ARG for a
 * null pointer, a size < 1 or S < R + 2. */
int fcd_baseline_group_glm(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                           const double *design, int64_t R, const uint16_t *perms, int64_t P, double *t, double *region,
                           double *null_max_t, double *null_max_region, int64_t *count_t, int64_t *count_region,
                           fcd_stream stream);
/* The bits of fcd_baseline_network_bits from the t^2 above; the side of FCD_TAIL_GREATER / _LESS is the sign of d_0.  perms may be
 * NULL with P = 1: the identity.  t (C,), nullable: the signed t of permutation 0.  Three launches.
 * Refusals as above and as fcd_baseline_network_bits: more than 1024 regions or P > 65535 * 32 FCD_ERR_UNSUPPORTED; perms == NULL
 * with P != 1, a threshold that is not finite and > 0, or an unknown tail FCD_ERR_ARG. */
int fcd_baseline_network_bits_glm(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                  const double *design, int64_t R, const uint16_t *perms, int64_t P, double threshold, int tail,
                                  uint32_t *bits, double *t, fcd_stream stream);
/* The components: per row of bits (B, W) the connected components of the graph on the Nreg regions whose edges are the set
 * bits; bits behind C in the last word are ignored.  A component's label is its smallest region, its extent its number of
 * connections.  component (B, Nreg), nullable: the label of each region's component, -1 for a region without an edge.
 * n_edges, max_extent, max_regions (B,): set bits, extent of the largest component, regions of the component with the most
 * regions (0 where no bit is set).  One workgroup per row, the row in LDS; integer atomics only, so two calls agree exactly.
 * One launch, no workspace.
 * FCD_ERR_SHAPE for a non-triangular C; FCD_ERR_UNSUPPORTED for more than 1024 regions (a row of bits is 64 KB there);
 * FCD_ERR_ARG for a null pointer other than component, or a size < 1. */
int fcd_graph_components(fcd_ctx *ctx, const uint32_t *bits, int64_t B, int64_t C, int32_t *component, int32_t *n_edges,
                         int32_t *max_extent, int32_t *max_regions, fcd_stream stream);
/* Component intensity (the second size of the NBS toolbox): the sum over a component's connections of the excess
 * e = max(|t| - threshold, 0).  Two entry points, each with one descriptor; a member an entry point does not name is not read.
 *
 * The bits pass with the excess of every set bit.  Which statistic: design != NULL the covariate form (design, R, perms; flags
 * must be 0; labels is not read); otherwise flags = 0 the pooled t on complete data and flags = FCD_BASELINE_MISSING |
 * FCD_BASELINE_WELCH the options (labels; design, R and perms are not read).  bits (P, W) and t (C,) of labelling 0 (nullable)
 * exactly as fcd_baseline_network_bits, _opt or _glm writes them: the same kernel shell, tile product, t^2 and compare.  excess
 * (P, 32 W) fp64: excess[p 32 W + c] = max(sqrt(t^2) - threshold, 0) WHERE BIT (p, c) IS SET, and nothing is stored anywhere
 * else -- the buffer may be uninitialised, what lies at an unset bit stays.  t = +/-inf (complete separation) gives +inf.  The
 * root is taken for set bits only.  A row equal to the observed labelling (the identity) gives the observed excess bit for bit.
 * Refusals: those of the bits entry point of the statistic, a null descriptor or excess, size != sizeof(fcd_network_excess_desc)
 * (FCD_ERR_ARG), flags with a design (FCD_ERR_UNSUPPORTED). */
typedef struct fcd_network_excess_desc {
    uint32_t size;             /* sizeof(fcd_network_excess_desc): the version of the layout */
    uint32_t flags;            /* FCD_BASELINE_MISSING | FCD_BASELINE_WELCH; 0 with a design */
    int64_t C, H, U, P;
    double threshold;          /* finite, > 0 */
    int32_t tail;              /* FCD_TAIL_* */
    int32_t R;                 /* design columns, 1 .. 9 */
    fcd_stream stream;         /* every launch goes here */
    /* device, read */
    const double *b;           /* (C, H) */
    const double *bt;          /* (C, U) */
    const uint8_t *labels;     /* (P, S), or NULL with P = 1: the observed labelling */
    const double *design;      /* (S, R), or NULL: no covariates */
    const uint16_t *perms;     /* (P, S), or NULL with P = 1: the identity */
    /* device, written */
    uint32_t *bits;            /* (P, W) */
    double *excess;            /* (P, 32 W), only where the bit is set */
    double *t;                 /* (C,) or NULL */
} fcd_network_excess_desc;
int fcd_baseline_network_excess(fcd_ctx *ctx, const fcd_network_excess_desc *d);
/* The components with a weight per set bit: bits (B, W), weights (B, 32 W) fp64, >= 0 (+inf allowed) where the bit is set and
 * read nowhere else.  component, n_edges, max_extent, max_regions as fcd_graph_components gives them.  intensity (B, Nreg),
 * nullable: the sum of the weights of a component's connections at the index of its label, 0.0 everywhere else;
 * max_intensity (B,): the largest of them, 0.0 where no bit is set.  Summation order: per region n the set bits of its row
 * (connections tri(n) .. tri(n) + n - 1) in ascending order, then per component these row sums over its regions in ascending
 * order; the maximum is an integer compare of the bit patterns.  No floating-point atomic: a row of bits gives the same
 * bits of result whatever B and wherever it stands.  One workgroup per row, 8 (Nreg + 1) bytes of LDS more than
 * fcd_graph_components (86 KB at 1024 regions, one workgroup per CU).  One launch, no workspace.
 * Refusals as fcd_graph_components; also a null descriptor, weights or max_intensity, size != sizeof(fcd_components_desc)
 * (FCD_ERR_ARG), flags != 0 (FCD_ERR_UNSUPPORTED). */
typedef struct fcd_components_desc {
    uint32_t size;             /* sizeof(fcd_components_desc): the version of the layout */
    uint32_t flags;            /* 0 */
    int64_t B;                 /* rows of bits */
    int64_t C;                 /* connections, triangular, at most 1024 regions */
    fcd_stream stream;         /* the launch goes here */
    /* device, read */
    const uint32_t *bits;      /* (B, W) */
    const double *weights;     /* (B, 32 W) */
    /* device, written */
    int32_t *component;        /* (B, Nreg) or NULL */
    int32_t *n_edges;          /* (B,) */
    int32_t *max_extent;       /* (B,) */
    int32_t *max_regions;      /* (B,) */
    double *intensity;         /* (B, Nreg) or NULL */
    double *max_intensity;     /* (B,) */
} fcd_components_desc;
int fcd_graph_components_weighted(fcd_ctx *ctx, const fcd_components_desc *d);

/* ---- variational updates ------------------------------------------------------------------ */
/* UnsharedRegionFit._update_lq_F, fit.py:157-174 (+ _eval_q_R_w 382-406). */
int fcd_vb_update_qF(fcd_ctx *ctx, const double *lq_R, const double *S_B, const double *lM,
                     const double *hyper, int64_t Nreg, int64_t U, double *lq_F, fcd_stream stream);
/* UnsharedRegionFit._update_lq_R, fit.py:176-198: Gauss-Seidel over regions, in place. */
int fcd_vb_update_qR(fcd_ctx *ctx, const double *lq_F, const double *lM, const double *hyper,
                     int64_t Nreg, int64_t U, int edge_mode, double *lq_R, fcd_stream stream);
/* The six terms of _eval_energy, fit.py:142-155 / 447-539, in its order:
 * terms6 = {E[ln p(f)], E[ln p(b|f)], E[ln p(r)], E[ln p(bt|f,r)], E[ln q_F], E[ln q_R]} (device).
 * energy = -t0 -t1 -t2 -t3 +t4 +t5.  Deterministic (fixed reduction order). */
int fcd_vb_energy(fcd_ctx *ctx, const double *lq_F, const double *lq_R, const double *S_B,
                  const double *lM, const double *hyper, int64_t Nreg, int64_t U, double *terms6,
                  fcd_stream stream);
/* _update_pi + _update_gamma, fit.py:208-220: out4 = {mean q_R[:,:,1], mean_c q_F[c,0,:]} (device);
 * when hyper != NULL also stores their logs there (the theta step without leaving the device). */
int fcd_vb_theta_step(fcd_ctx *ctx, const double *lq_F, const double *lq_R, int64_t Nreg, int64_t U,
                      double *out4, double *hyper, fcd_stream stream);

/* ---- (eta, epsilon) step: objective and analytic gradient --------------------------------------------
 * The reference sketches a bounded minimisation of -E_lM over (eta, epsilon) (fit.py:222-286) that cannot run there
 * (fit.py:239 calls an undefined name); its derivative helpers are complete (fit.py:600-697).  For weights
 * W (C, U, 3, 3) >= 0 these return out3 = {S, dS/d eta, dS/d epsilon} (device), S = sum W[c,u,k,l] ln M_kl(bt_cu):
 *   W = q_F[c,k] w_l(c,u)            -> S = E_lM (fit.py:489-511), energy derivative = -dS  (variational fit)
 *   W = pooled chain counts          -> Monte-Carlo EM objective of the sampler
 * theta12_host as in fcd_lik_tables.  Deterministic. */
int fcd_theta_sub_weights_vb(fcd_ctx *ctx, const double *lq_F, const double *lq_R, int64_t Nreg, int64_t U, double *W,
                             fcd_stream stream);
/* W[c,u,k,l] (+)= number of this rank's chains with f_c = k and mixture case l at (c,u)  (accumulate != 0: add).
 * The counts of fcd_gibbs_pair_tally, written as fp64 (exact integers). */
int fcd_gibbs_pair_counts(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U,
                          int64_t G, int accumulate, double *W, fcd_stream stream);
int fcd_theta_sub_objective(fcd_ctx *ctx, const double *bt, const double *W, int64_t C, int64_t U,
                            const double *theta12_host, double *out3, fcd_stream stream);
/* The FULL theta_sub objective the reference intends but comments out (fit.py:232-237 bounds, :250-251 / :266-267 pack
 * and unpack of mu and sigma^2, :282 the E[ln p(b | f)] term):
 *   S = sum_{c,k} wF[c,k] sum_h ln N(b[c,h]; mu_k, sigma_k) + sum W[c,u,k,l] ln M_kl(bt[c,u]),   wF[c,k] = sum_l W[c,0,k,l]
 * out9 = {S, dS/d eta, dS/d epsilon, dS/d mu_0..2, dS/d (sigma^2)_0..2} (device): the true gradient of S in the
 * reference's own parametrisation (it packs sigma ** 2).  Forms: fit.py:542-569, 572-597 (without quirk Q8, which
 * lives in a helper the objective never calls), 709-733; doc/methods.rst:715-944.  b == NULL leaves the first sum out.
 * Deterministic. */
int fcd_theta_full_objective(fcd_ctx *ctx, const double *b, const double *bt, const double *W, int64_t C, int64_t H,
                             int64_t U, const double *theta12_host, double *out9, fcd_stream stream);
/* The two objectives with flags.  With FCD_DATA_NAN_MISSING an item with NaN bt adds nothing to S or its gradient (its
 * M = 1 depends on no parameter), and a NaN b adds nothing to the mu / sigma^2 terms. */
int fcd_theta_sub_objective_ex(fcd_ctx *ctx, const double *bt, const double *W, int64_t C, int64_t U,
                               const double *theta12_host, int flags, double *out3, fcd_stream stream);
int fcd_theta_full_objective_ex(fcd_ctx *ctx, const double *b, const double *bt, const double *W, int64_t C, int64_t H,
                                int64_t U, const double *theta12_host, int flags, double *out9, fcd_stream stream);

/* ---- many-chain collapsed Gibbs sampler ---------------------------------------------------
 * Build-defined (the reference ships only the variational fitter, doc/methods.rst:236-239).  Its two
 * conditionals are the reference's updates at one-hot q:
 *   p(f_c = k | r)      = softmax_k of fit.py:170-173 with q_R one-hot
 *   p(r_nu = j | f, r)  = softmax_j of fit.py:187-194 with q_F, q_R one-hot
 * Randomness: Philox4x32-10, key = seed, counter = (site, global chain id, sweep, kind), so a chain's
 * trajectory depends only on (seed, chain id): not on G, the launch geometry or the number of GPUs. */
int fcd_gibbs_state_size(int64_t Nreg, int64_t U, int64_t G, size_t *f_bytes, size_t *r_bytes);
/* f ~ Uniform{0,1,2}, r ~ Bernoulli(pi) from the counter RNG (kinds 0, 1). */
int fcd_gibbs_init(fcd_ctx *ctx, uint8_t *f_state, uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                   int64_t chain0, uint64_t seed, double pi, fcd_stream stream);
/* Edge-major DIFFERENCE table for the f step: lMf (C, U, 3, 2), lMf[c][u][l][k-1] = lM[c,u,k,l] - lM[c,u,0,l]
 * (the log-odds of type k against type 0 contributed by patient u in mixture case l).  48*C*U bytes. */
int fcd_gibbs_edge_tables(fcd_ctx *ctx, const double *lM, int64_t Nreg, int64_t U, double *lMf, fcd_stream stream);
/* Redraw every f_c of every chain given r (edges are conditionally independent).  With lMf only the two
 * log-odds against type 0 are accumulated (one 16-byte read + two adds per term); lMf == NULL runs the
 * kernel that accumulates the three sums of fit.py:170-173 from lM directly.
 * Alignment: f_state and lMf must be 16-byte aligned (ALIGNMENT, top of this file). */
int fcd_gibbs_f_step(fcd_ctx *ctx, const double *S_B, const double *lM, const double *lMf, const double *hyper,
                     uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                     int64_t chain0, uint64_t seed, int64_t sweep, fcd_stream stream);
/* Region-major DIFFERENCE table for the r step: lMd (U, Nreg, Nreg, 3, 2),
 *   lMd[u][n][m][k][t] = t ? lM[c,u,k,1] - lM[c,u,k,2] : lM[c,u,k,2] - lM[c,u,k,0],  c = edge(n, m),
 * the contribution of region m (state t) to s1 - s0 of fit.py:187-194 when f_c = k; edge() = the
 * ordered-pair edge id of `edge_mode` (zeros at m == n).  Built once per table build; 48*U*Nreg*Nreg bytes. */
int fcd_gibbs_region_tables(fcd_ctx *ctx, const double *lM, int64_t Nreg, int64_t U, int edge_mode, double *lMd,
                            fcd_stream stream);
/* Redraw every r_nu of every chain given f, regions in order 0..Nreg-1 (systematic scan; patients
 * and chains in parallel).  With lMd (made with the SAME edge_mode) the blocked path runs: panel kernels
 * stream lMd rows through LDS, small diagonal kernels resolve the in-order dependence (only s1 - s0
 * is formed, as a sum of table differences: same conditional, one add per term).  lMd == NULL
 * selects the generic kernel that gathers from lM directly (any shape, much slower).
 * Alignment: f_state and lMd must be 16-byte aligned (ALIGNMENT, top of this file). */
int fcd_gibbs_r_step(fcd_ctx *ctx, const double *lM, const double *lMd, const double *hyper,
                     const uint8_t *f_state, uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                     int64_t chain0, uint64_t seed, int64_t sweep, int edge_mode, fcd_stream stream);
/* n_sweeps x (f step, r step), sweeps numbered sweep0, sweep0+1, ...: fcd_gibbs_run's loop without M-step or counters.
 * When counts != NULL the pooled statistics of the LAST sweep are stored there (fcd_gibbs_stats: this rank's own).
 * Waits for the stream as fcd_gibbs_run does (below) in a call that builds the f pass's records.
 * Alignment: f_state, lMf and lMd must be 16-byte aligned (ALIGNMENT, top of this file). */
int fcd_gibbs_sweeps(fcd_ctx *ctx, const double *S_B, const double *lM, const double *lMf, const double *lMd,
                     const double *hyper, uint8_t *f_state, uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, int64_t chain0,
                     uint64_t seed, int64_t sweep0, int64_t n_sweeps, int edge_mode, int64_t *counts,
                     fcd_stream stream);
/* Pooled sufficient statistics over the G chains (the all-reduce payload):
 * counts[0..7] = {sum r, #f=0, #f=1, #f=2, G, 0, 0, 0} (int64, device, overwritten).  fcd_gibbs_tally with counts only.
 * Alignment: f_state must be 16-byte aligned (ALIGNMENT, top of this file). */
int fcd_gibbs_stats(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U,
                    int64_t G, int64_t *counts, fcd_stream stream);
/* M-step for (pi, gamma) from pooled counts (after the cross-GPU all-reduce): the sample version of
 * fit.py:208-220.  Writes hyper[0..4]; pi is kept inside [1/(2n), 1-1/(2n)], n = G*Nreg*U sites. */
int fcd_gibbs_mstep(fcd_ctx *ctx, const int64_t *counts, int64_t Nreg, int64_t U, double *hyper,
                    fcd_stream stream);
/* Running marginal counts over sweeps AND chains: cnt_f (C,3) += [f_c = k], cnt_r (Nreg,U) += r_nu
 * (uint32, device, wrapping); posterior marginals = counts / (sweeps * G).  fcd_gibbs_tally with counters only.
 * Alignment: f_state must be 16-byte aligned (ALIGNMENT, top of this file). */
int fcd_gibbs_accumulate(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg,
                         int64_t U, int64_t G, uint32_t *cnt_f, uint32_t *cnt_r, fcd_stream stream);
/* fcd_gibbs_stats and fcd_gibbs_accumulate in ONE pass over the state and ONE launch (the pooled sums are kept in
 * accumulators of the context that the kernel itself puts back to zero: no memset; the two entry points are this launch
 * with one half of its output):
 * counts (nullable) is overwritten as by fcd_gibbs_stats; cnt_f / cnt_r (both or neither) are incremented.
 * Alignment: f_state must be 16-byte aligned (ALIGNMENT, top of this file). */
int fcd_gibbs_tally(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U,
                    int64_t G, int64_t *counts, uint32_t *cnt_f, uint32_t *cnt_r, fcd_stream stream);
/* The sampler loop of one rank between two exchanges of pooled statistics -- what the fit loop calls:
 *   for i in 0 .. n_sweeps-1:   f pass, r pass (sweep number sweep0 + i), then ONE tally launch that
 *     - adds the state to the marginal counters cnt_f / cnt_r (nullable, both or neither) when sweep0 + i >= accumulate_from,
 *     - when mstep_every > 0 and (i + 1) % mstep_every == 0 runs the (pi, gamma) M-step of fcd_gibbs_mstep on THIS
 *       rank's pooled counts and writes hyper (single-rank use; with several ranks pass 0, all-reduce `counts` and
 *       call fcd_gibbs_mstep),
 *     - makes the packed r words of the next f pass.
 *   counts (nullable) receives the pooled statistics of the LAST sweep.
 * 4 launches per sweep (f pass; packing, which also carries the f half of the tally in workgroups of its own; pipelined r
 * pass; the rest of the tally: r counts, slot words, M-step) where the pipelined r pass fits the device at once, else
 * ceil(Nreg/16) + 4 (one launch per block step).
 * NOT fully asynchronous: a call that builds the f pass's pair records (knob "f_records": by default a call with at least
 * F_REC_MIN_SWEEPS pair-tile sweeps) queues the build and the first sweep, then reads the build's hint -- has the table
 * decided tiles? -- from a pinned word before it queues the second sweep.  The host polls that word, so it waits until the
 * stream has run everything queued before the build, the build and its hint kernel (whatever the caller queued on the
 * stream before the call included); after two seconds it falls back to hipStreamSynchronize.  Only this stream is waited
 * for.  A call without a record build (one sweep, knob f_records = 1, a shape without the pair-tile f pass) returns without
 * waiting.
 * Alignment: f_state, lMf and lMd must be 16-byte aligned (ALIGNMENT, top of this file). */
int fcd_gibbs_run(fcd_ctx *ctx, const double *S_B, const double *lM, const double *lMf, const double *lMd,
                  double *hyper,
                  uint8_t *f_state, uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, int64_t chain0, uint64_t seed,
                  int64_t sweep0, int64_t n_sweeps, int edge_mode, int64_t mstep_every, int64_t accumulate_from,
                  int64_t *counts, uint32_t *cnt_f, uint32_t *cnt_r, fcd_stream stream);
/* ---- connection-level posteriors (T and F~ of each connection and patient) -------------------------------
 * Both fitters integrate T and F~ out into M_kl (doc/methods.rst:248-349); given f_c = k, the mixture case l of the
 * TRUE endpoints of c (both edge-id modes) and bt_cu their law is closed-form, so a fit only has to average three
 * tables over its posterior of (f_c, l_cu).
 *
 * Counts of (f_c = k, l_cu = l) over chains: acc (C, U, 3, 3) uint32, acc[c,u,k,l] += #{chains with f_c = k and mixture
 * case l at (c,u)} of the current state (the integers fcd_gibbs_pair_counts gives as doubles). */
int fcd_gibbs_pair_tally(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U,
                         int64_t G, uint32_t *acc, fcd_stream stream);
/* Attach acc (C, U, 3, 3) uint32 for shape (Nreg, U) to the context (no device work; acc == NULL detaches): from then on
 * every sweep s of fcd_gibbs_run with s >= accumulate_from and (s - accumulate_from) % every == 0 adds its end-of-sweep
 * state to acc (one extra launch after the sweep's tally).  fcd_gibbs_run refuses another shape while it is attached.
 * The caller keeps sweeps x G below 2^32. */
int fcd_gibbs_set_pair_accumulator(fcd_ctx *ctx, uint32_t *acc, int64_t Nreg, int64_t U, int64_t every);
/* p_T (C, U) = P(T = 1), p_F_tilde (C, U, 3) = P(F~ = j), p_changed (C, U) = P(F~ != F) for weights over (k, l) of
 *   counts != NULL:          counts (C, U, 3, 3) uint32, normalised per (c, u) by their sum (sampler), or
 *   counts == NULL:          q_F[c,k] w_l(c,u) from lq_F (C, 1, 3) and lq_R (Nreg, U, 2) (variational fit),
 * bt (C, U) and theta12_host as in fcd_lik_tables.  fp64; finite where all three densities underflow. */
int fcd_conn_posterior(fcd_ctx *ctx, const double *bt, int64_t Nreg, int64_t U, const double *theta12_host,
                       const uint32_t *counts, const double *lq_F, const double *lq_R, double *p_T, double *p_F_tilde,
                       double *p_changed, fcd_stream stream);
/* fcd_conn_posterior with flags.  With FCD_DATA_NAN_MISSING the closed forms take N_j = 1 at a NaN bt[c,u]: the prior
 * law of T and F~ given (k, l), averaged over the same weights.  Observed items are unchanged. */
int fcd_conn_posterior_ex(fcd_ctx *ctx, const double *bt, int64_t Nreg, int64_t U, const double *theta12_host,
                          const uint32_t *counts, const double *lq_F, const double *lq_R, int flags, double *p_T,
                          double *p_F_tilde, double *p_changed, fcd_stream stream);
/* ---- anomalous-region counts (how many regions of a patient, in how many patients a region) ---------------------
 * The law of sum_n r_nu and of sum_u r_nu depends on the joint law of the sites, not on their marginals.
 *
 * Histograms over chains of one state: hist_patient (U, Nreg+1) uint32, hist_patient[u][k] += #{chains with
 * sum_n r_nu = k}; hist_region (Nreg, U+1) uint32, hist_region[n][k] += #{chains with sum_u r_nu = k}.  Both from one
 * read of r_bits.  Nreg <= 1023 and U <= 512, else FCD_ERR_UNSUPPORTED. */
int fcd_gibbs_count_tally(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, uint32_t *hist_patient,
                          uint32_t *hist_region, fcd_stream stream);
/* Attach both histograms for shape (Nreg, U) to the context (no device work; both NULL detaches), with the semantics of
 * fcd_gibbs_set_pair_accumulator: every sweep s of fcd_gibbs_run with s >= accumulate_from and
 * (s - accumulate_from) % every == 0 adds its end-of-sweep state (two extra launches after the sweep's tally, after the
 * pair accumulator's when both are attached; fcd_gibbs_run grows the context's scratch for them before its loop).
 * fcd_gibbs_run refuses another shape while they are attached.  The caller keeps sweeps x G below 2^32. */
int fcd_gibbs_set_count_accumulator(fcd_ctx *ctx, uint32_t *hist_patient, uint32_t *hist_region, int64_t Nreg, int64_t U,
                                    int64_t every);
/* The mean-field law of the same counts under q_R (sites independent: Poisson-binomial), fp64:
 * p_patient (U, Nreg+1), p_patient[u][k] = P(sum_n r_nu = k); p_region (Nreg, U+1), p_region[n][k] = P(sum_u r_nu = k).
 * q_nu = P(r_nu = 1) from lq_R (Nreg, U, 2), normalised in log space (lq_R need not be normalised).  Exact convolution
 * recursion; q = 0 and q = 1 give exact point masses.  Nreg, U <= 4095, else FCD_ERR_UNSUPPORTED. */
int fcd_vb_count_posterior(fcd_ctx *ctx, const double *lq_R, int64_t Nreg, int64_t U, double *p_patient, double *p_region,
                           fcd_stream stream);
/* ---- anomalous-region counts over sets of regions (networks of an atlas) --------------------------------------------
 * For user-given sets S_0 .. S_{J-1} of regions: the law of sum_{n in S_j} r_nu and of #{u : r_nu = 1 for some n in S_j}.
 * Both depend on the joint law of a patient's sites; the set of all regions gives fcd_gibbs_count_tally's hist_patient,
 * a singleton {n} its hist_region[n].
 *
 * The sets of the context, CSR in HOST memory: offsets_host (J + 1, offsets[0] = 0), members_host (offsets[J]), the members
 * of a set strictly increasing (no duplicates).  Sets may overlap and may repeat.  Everything is checked here, on the host:
 * FCD_ERR_ARG for a null pointer, J < 1, offsets[0] != 0, an empty set, a negative member or members that do not increase;
 * FCD_ERR_UNSUPPORTED for a set of more than 1023 members or J > 1024.  The context copies both arrays into a device buffer
 * it owns and frees (it synchronises).  J = 0 with both arrays NULL clears.  Refused with FCD_ERR_ARG while the region-set
 * accumulator is attached, or the patient-group or patient-trait accumulator with the sets as rows. */
int fcd_region_sets_set(fcd_ctx *ctx, const int32_t *offsets_host, const int32_t *members_host, int64_t J);
/* Histograms over chains of one state, with S_max the size of the largest set:
 *   hist_set (J, U, S_max+1) uint32, hist_set[j][u][k] += #{chains with sum_{n in S_j} r_nu = k}; the bins k > |S_j| are
 *   never touched;
 *   hist_prev (J, U+1) uint32, hist_prev[j][k] += #{chains with #{u : r_nu = 1 for some n in S_j} = k}.
 * Chains beyond G in the last word never count.  Two launches; the scratch, (J U + J) rows of ceil(G/64) * 64 uint16, is the
 * count tally's, grown on demand.  FCD_ERR_ARG without sets, FCD_ERR_SHAPE if the largest member is >= Nreg,
 * FCD_ERR_UNSUPPORTED for U > 512 or a scratch above 1 GiB. */
int fcd_gibbs_region_set_tally(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, uint32_t *hist_set,
                               uint32_t *hist_prev, fcd_stream stream);
/* Attach both histograms for shape (Nreg, U) and the context's CURRENT sets (no device work; both NULL detaches), with the
 * semantics of fcd_gibbs_set_count_accumulator: every sweep s of fcd_gibbs_run with s >= accumulate_from and
 * (s - accumulate_from) % every == 0 adds its end-of-sweep state (two extra launches after the sweep's tally, after the other
 * accumulators'; fcd_gibbs_run grows the scratch before its loop and refuses one above 1 GiB).  Refusals as
 * fcd_gibbs_region_set_tally's; fcd_gibbs_run refuses another shape while they are attached, and fcd_region_sets_set
 * refuses to change the sets.  fcd_gibbs_sweeps never adds to them.  The caller keeps sweeps x G below 2^32. */
int fcd_gibbs_set_region_set_accumulator(fcd_ctx *ctx, uint32_t *hist_set, uint32_t *hist_prev, int64_t Nreg, int64_t U,
                                         int64_t every);
/* ---- anomaly prevalence over groups of patients, and contrasts between two groups -------------------------------------
 * For user-given groups g_0 .. g_{J-1} of patients and every row rho: the law of k_j = #{u in g_j : the row's indicator is 1
 * in patient u}; for every contrast (a, b) of two DISJOINT groups the joint law of (k_a, k_b).  The rows are the Nreg regions
 * (indicator r_nu) and, if the groups were set with_region_sets, after them the context's J_S region sets (indicator "some n
 * in S has r_nu = 1"): R = Nreg + J_S.  Patients are coupled through f, so neither law follows from per-patient marginals.
 * The group of all patients gives fcd_gibbs_count_tally's hist_region at a region row and fcd_gibbs_region_set_tally's
 * hist_prev at a set row.
 *
 * The groups of the context, CSR in HOST memory: offsets_host (J + 1, offsets[0] = 0), members_host (offsets[J]), the members
 * of a group strictly increasing; groups may overlap.  contrasts_host: P pairs (a, b) of group indices (NULL with P = 0).
 * Everything is checked here, on the host: FCD_ERR_ARG for a null pointer, J < 1, P < 0, offsets[0] != 0, an empty group, a
 * negative member, members that do not increase, a contrast that names a group outside [0, J) or one group twice, or whose
 * groups overlap; FCD_ERR_UNSUPPORTED for a member >= 512 (U <= 512), J > 64, P > 64, or a contrast of more than 16384 joint
 * bins (|a|+1)(|b|+1) -- 64 KiB of uint32, the LDS of the one workgroup that owns a joint row; the message names the contrast.
 * The context copies the CSR, the contrasts, a bit mask over u per group (8 words, of which the kernels read ceil(U/64)) and
 * the contrasts' bin offsets into a device buffer it owns and frees (it synchronises).  J = 0 with offsets, members and
 * contrasts NULL and P = 0 clears.  Refused with FCD_ERR_ARG while the patient-group accumulator is attached. */
int fcd_patient_groups_set(fcd_ctx *ctx, const int32_t *offsets_host, const int32_t *members_host, int64_t J,
                           const int32_t *contrasts_host, int64_t P, int with_region_sets);
/* Histograms over chains of one state, with Umax the size of the largest group:
 *   hist_group (J, R, Umax+1) uint32, hist_group[j][rho][k] += #{chains with k_j(rho) = k}; the bins k > |g_j| are never
 *   touched;
 *   hist_joint, flat uint32: block p of contrast (a, b) is (R, |a|+1, |b|+1) and starts at word R * boff[p],
 *   boff[p] = sum_{q < p} (|a_q|+1)(|b_q|+1); hist_joint[R boff[p] + (rho (|a|+1) + k_a)(|b|+1) + k_b] += #{chains with that
 *   pair of counts}.  R * boff[P] words in all; with P = 0 a placeholder of one word, never touched.
 * Chains beyond G in the last word never count, and patients beyond U in the last 64-patient chunk read as 0.  Two launches;
 * the scratch, J R rows of ceil(G/64) * 64 uint16, is the count tally's, grown on demand.  FCD_ERR_ARG without groups, or
 * without region sets when the groups were set with them; FCD_ERR_SHAPE if the largest member of a group is >= U or the
 * largest member of a region set is >= Nreg; FCD_ERR_UNSUPPORTED for U > 512 or a scratch above 1 GiB. */
int fcd_gibbs_patient_group_tally(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                                  uint32_t *hist_group, uint32_t *hist_joint, fcd_stream stream);
/* Attach both histograms for shape (Nreg, U) and the context's CURRENT groups (and region sets, if they are rows) -- no device
 * work; both NULL detaches --, with the semantics of fcd_gibbs_set_region_set_accumulator: every sweep s of fcd_gibbs_run with
 * s >= accumulate_from and (s - accumulate_from) % every == 0 adds its end-of-sweep state (two extra launches, after the other
 * accumulators'; fcd_gibbs_run grows the scratch before its loop and refuses one above 1 GiB).  Refusals as
 * fcd_gibbs_patient_group_tally's; while attached fcd_gibbs_run refuses another shape, fcd_patient_groups_set refuses to
 * change the groups and, with the sets as rows, fcd_region_sets_set to change the sets.  fcd_gibbs_sweeps never adds to them.
 * The caller keeps sweeps x G below 2^32. */
int fcd_gibbs_set_patient_group_accumulator(fcd_ctx *ctx, uint32_t *hist_group, uint32_t *hist_joint, int64_t Nreg, int64_t U,
                                            int64_t every);
/* ---- anomalies against an ordered patient trait: rank-sum (AUC) laws per row ------------------------------------------
 * For Q traits of the patients (severity, duration, dose ...) and every row rho of the patient-group histograms (the Nreg
 * regions and, if the traits were set with_region_sets, the context's J_S region sets after them: R = Nreg + J_S), the law of
 * the Mann-Whitney statistic between the patients that are anomalous at the row and those that are not.  The caller ranks
 * trait q over its n_q known patients and passes doubled, centred midranks a_u = 2 midrank_u - (n_q + 1): integers in
 * [-(n_q - 1), n_q - 1] that sum to 0, tied values sharing a midrank.  A chain state gives, per (q, rho),
 *     k = #{u known : indicator 1},    A = sum_{u known, indicator 1} a_u,
 * and where 0 < k < n_q (the state is DEFINED)  AUC = 1/2 + A / (2 k (n_q - k)) = P(an anomalous patient has the higher
 * trait) + P(tie) / 2;  A + k (n_q - k) = 2 U_stat >= 0.  All of it is integer arithmetic.
 *
 * The traits of the context, in HOST memory: scores_host int32 (Q, U), known_host uint8 (Q, U) (non-zero: known).  Everything
 * a kernel indexes with is checked here: FCD_ERR_ARG for a null pointer, Q < 1, U < 1, a trait with n_q < 2, a score where the
 * trait is not known, |score| > n_q - 1, scores that do not sum to 0 or known patients that all have one score;
 * FCD_ERR_UNSUPPORTED for Q > 16 or U > 512.  The context copies the words 2 score + known and the n_q into a device buffer it
 * owns and frees (it synchronises).  Q = 0 with both arrays NULL clears.  Refused with FCD_ERR_ARG while the patient-trait
 * accumulator is attached. */
int fcd_patient_traits_set(fcd_ctx *ctx, const int32_t *scores_host, const uint8_t *known_host, int64_t Q, int64_t U,
                           int with_region_sets);
/* Histograms over chains of one state, with Umax = max_q n_q and NB = 128:
 *   trait_hist (Q, R, Umax+1 + NB + 3) uint32: [k] += #{chains with that k}, k <= n_q (the bins beyond n_q are never touched);
 *   [Umax+1 + b] += #{defined chains with min(NB-1, floor(NB (A + d) / (2 d))) = b}, d = k (n_q - k): AUC bins of width 1/NB;
 *   the last three words += #{defined chains with A < 0, A = 0, A > 0};
 *   trait_sum (Q, R, Umax+1) int64: [k] += sum of A over the chains with that k.
 * Chains beyond G in the last word never count.  Two launches; the scratch, Q R rows of ceil(G/64) * 64 (uint16, int32) pairs,
 * is the count tally's, grown on demand.  FCD_ERR_ARG without traits, or without region sets when the traits were set with
 * them; FCD_ERR_SHAPE if U is not the U of the traits or the largest member of a region set is >= Nreg; FCD_ERR_UNSUPPORTED
 * for a scratch above 1 GiB. */
int fcd_gibbs_patient_trait_tally(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                                  uint32_t *trait_hist, int64_t *trait_sum, fcd_stream stream);
/* Attach both buffers for shape (Nreg, U) and the context's CURRENT traits (and region sets, if they are rows) -- no device
 * work; both NULL detaches --, with the semantics of fcd_gibbs_set_patient_group_accumulator: every sweep s of fcd_gibbs_run
 * with s >= accumulate_from and (s - accumulate_from) % every == 0 adds its end-of-sweep state (two extra launches, after the
 * other accumulators'; fcd_gibbs_run grows the scratch before its loop and refuses one above 1 GiB).  Refusals as
 * fcd_gibbs_patient_trait_tally's; while attached fcd_gibbs_run refuses another shape, fcd_patient_traits_set refuses to change
 * the traits and, with the sets as rows, fcd_region_sets_set to change the sets.  fcd_gibbs_sweeps never adds to them.  The
 * caller keeps sweeps x G below 2^32. */
int fcd_gibbs_set_patient_trait_accumulator(fcd_ctx *ctx, uint32_t *trait_hist, int64_t *trait_sum, int64_t Nreg, int64_t U,
                                            int64_t every);
/* ---- co-anomaly (which regions are anomalous together, which patients share anomalous regions) -------------------
 * Second moments of the joint law of the sites, which the marginals do not give.
 *
 * Counts over chains of one state, both symmetric and written in full:
 *   region_pairs (Nreg, Nreg) uint32, region_pairs[n][m] += #{(chain, u) with r_nu = r_mu = 1};
 *   patient_pairs (U, U) uint32, patient_pairs[u][v] += #{(chain, n) with r_nu = r_nv = 1}.
 * The diagonals are sum_u r_nu and sum_n r_nu over chains.  Chains beyond G in the last word never count.  One launch,
 * no scratch.  Any shape the sampler takes (U = 1 included). */
int fcd_gibbs_coanomaly_tally(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                              uint32_t *region_pairs, uint32_t *patient_pairs, fcd_stream stream);
/* Attach both matrices for shape (Nreg, U) to the context (no device work; both NULL detaches), with the semantics of
 * fcd_gibbs_set_count_accumulator: every sweep s of fcd_gibbs_run with s >= accumulate_from and
 * (s - accumulate_from) % every == 0 adds its end-of-sweep state (one extra launch after the sweep's tally, after the
 * pair and count accumulators' when they are attached).  fcd_gibbs_run refuses another shape while they are attached.
 * The caller keeps sweeps x G x max(Nreg, U) below 2^32. */
int fcd_gibbs_set_coanomaly_accumulator(fcd_ctx *ctx, uint32_t *region_pairs, uint32_t *patient_pairs, int64_t Nreg,
                                        int64_t U, int64_t every);
/* The same two matrices per chain if the sites were independent with q_nu = P(r_nu = 1) from lq_R (Nreg, U, 2),
 * normalised in log space (lq_R need not be normalised; q = 0 and q = 1 exact), fp64:
 *   region (Nreg, Nreg):  sum_u q_nu q_mu off the diagonal, sum_u q_nu on it;
 *   patient (U, U):       sum_n q_nu q_nv off the diagonal, sum_n q_nu on it.
 * Every entry is summed in index order: results repeat bit for bit. */
int fcd_vb_coanomaly(fcd_ctx *ctx, const double *lq_R, int64_t Nreg, int64_t U, double *region, double *patient,
                     fcd_stream stream);
/* ---- scoring new patients against a fitted model (UnsharedRegionFit.score) -------------------------------------------
 * Given F and theta the patients are independent, so a new patient is scored with the fit's template held: the fit itself
 * is never changed.
 *
 * Per-patient split of the variational energy terms that involve patients, for lq_F (C, 1, 3), lq_R (Nreg, U, 2) and the
 * patients' table lM (C, U, 3, 3):  out4 (U, 4) = {E_lM[u], E_lp_R[u], E_lq_R[u], elbo[u] = E_lM + E_lp_R - E_lq_R}, with
 *   E_lM[u] = sum_c sum_k q_F[c,k] sum_l w_l(c,u) lM[c,u,k,l]  (true endpoints of c, as in fcd_vb_energy's E_lM term),
 * E_lp_R / E_lq_R the terms of fit.py:486 / :539 restricted to patient u.  elbo[u] is a lower bound on
 * E_{q_F} log p(bt_u | F).  Sums over u are fcd_vb_energy's terms 3, 2 and 5.  fp64, bitwise repeatable, and patient u's
 * numbers do not depend on the other patients of the call.  Uses the context's workspace. */
int fcd_vb_patient_elbo(fcd_ctx *ctx, const double *lq_F, const double *lq_R, const double *lM, const double *hyper,
                        int64_t Nreg, int64_t U, double *out4, fcd_stream stream);
/* One step of annealed importance sampling over r with the chains' f held (symmetric edge ids: the true endpoints of c):
 *   l_gu = sum_c lM[c, u, f_gc, l(r_gnu, r_gmu)]  at the current state (mixture case l as in fcd_gibbs_logjoint),
 *   w[g, u] += (beta - beta_prev) l_gu            w (G, U) fp64, device,
 *   lM_beta = beta * lM                           (C, U, 3, 3), the working table the next fcd_gibbs_region_tables and
 *                                                 fcd_gibbs_r_step read (NULL: not written; must not alias lM or w).
 * Started from r drawn from the prior (beta = 0) and followed, at every beta_t of a ladder ending at 1, by one r pass on
 * the beta_t table, exp(w[g, u]) is an unbiased estimate of p(bt_u | f_g).  Two launches; uses the context's workspace.
 * Alignment: f_state must be 16-byte aligned (ALIGNMENT, top of this file). */
int fcd_score_ais_step(fcd_ctx *ctx, const double *lM, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U,
                       int64_t G, double beta_prev, double beta, double *w, double *lM_beta, fcd_stream stream);
/* The per-patient fold of the AIS weights w (G, U): out4 (U, 4) = {m = max_g w[g,u], sum_g exp(w - m), sum_g exp(2 (w - m)),
 * G} (sums 0 when m = -inf), the numbers that pool over ranks into log-mean-exp, its standard error and the effective
 * sample size.  Chains in a fixed order: bitwise repeatable. */
int fcd_score_ais_finish(fcd_ctx *ctx, const double *w, int64_t U, int64_t G, double *out4, fcd_stream stream);
/* ---- model evidence by annealed importance sampling over (f, r) (UnsharedRegionFit.log_evidence) -----------------------
 * log Z = log sum_{f,r} p(f; gamma) p(r; pi) exp(E(f, r)),  E = sum_c S_B[c, f_c] + sum_{c,u} lM[c, u, f_c, l(r_nu, r_mu)]
 * (symmetric edge ids: the true endpoints of c), is log p(b, bt | theta).  A ladder 0 = beta_0 < ... < beta_T = 1 starts
 * from a draw of the prior (one sweep on all-zero tables) and at every rung adds (beta_t - beta_{t-1}) E to each chain's
 * log-weight, then sweeps once on the beta_t-scaled tables (fcd_gibbs_sweeps): exp(w_g) is an unbiased estimate of Z.
 *
 * One rung's weight update:  w[g] += (beta - beta_prev) E_g  at the current state, w (G,) fp64, device.  The table is staged
 * through LDS once per 32 chain words (not once per chain word as in fcd_score_ais_step).  fp64, fixed reduction order:
 * bitwise repeatable, and chain g's number does not depend on the other chains of the call.  Two launches; uses the
 * context's workspace. */
int fcd_evidence_energy(fcd_ctx *ctx, const double *S_B, const double *lM, const uint8_t *f_state, const uint64_t *r_bits,
                        int64_t Nreg, int64_t U, int64_t G, double beta_prev, double beta, double *w, fcd_stream stream);
/* dst[j][i] = beta * src[j][i], i < n[j], for n_tables (1 to 8) tables in ONE launch: the working tables of a rung (S_B, lM
 * and the two difference tables, which are linear in lM).  src, dst, n are host arrays of device pointers / element counts;
 * dst[j] may be src[j].  beta = 1 copies bit for bit.  An all-zero table is the caller's zero fill, not beta = 0
 * (0 * -inf is NaN).
 * Alignment: the path is chosen by the address -- src[j] and dst[j] both 16-byte aligned take the 16-byte path,
 * anything else the 8-byte one, with the same bits (ALIGNMENT, top of this file). */
int fcd_evidence_temper(fcd_ctx *ctx, double beta, int64_t n_tables, const double *const *src, double *const *dst,
                        const int64_t *n, fcd_stream stream);
/* ---- patient or control: the two per-chain log-likelihoods of new subjects (UnsharedRegionFit.membership) ----------------
 * For subjects x (C, U) fp64 (device, the fit's edge order), theta (12 doubles, host) and the packed chain state:
 *   out_control[g, u] = sum_c ln N(x_cu; mu_k, sigma_k),  k = f_c of chain g              (G, U) fp64, device
 *   out_patient[g, u] = sum_c ln M_{k, l}(x_cu),          l = mixture case of chain g's (r_n, r_m) at the true endpoints of c
 *                                                         (symmetric edge ids), the entries of lM;  NULL: not computed
 * r_bits has r_cols columns per region: r_cols = U, one r column per subject (r_bits (GW, Nreg, U)), or r_cols = 1, ONE column
 * for every subject (r_bits (GW, Nreg, 1): the shared-region model's population r).  r_bits may be NULL when out_patient is.
 * flags: FCD_DATA_NAN_MISSING -- a NaN x is unobserved and adds 0 to both sides; without it NaN propagates.  A density that
 * underflows gives -inf, as in lM.  No (C, U, 3, 3) table is made: per (c, u) the 3 + 9 logs are computed once into LDS, by the
 * arithmetic of the table kernels, and looked up by the chains.  fp64, fixed reduction order (edge slices that depend on
 * (Nreg, U) and the device alone): bitwise repeatable, and chain g's numbers do not depend on G or on the other chains of
 * the call.  Fold the matrices with fcd_score_ais_finish.  Two launches; uses the context's workspace
 * (slices x U x 64 ceil(G / 64) doubles per side). */
int fcd_member_loglik(fcd_ctx *ctx, const double *x, const double *theta, const uint8_t *f_state, const uint64_t *r_bits,
                      int64_t Nreg, int64_t U, int64_t G, int r_cols, int flags, double *out_control, double *out_patient,
                      fcd_stream stream);
/* log p(f, r, b, bt; theta) of each chain = minus the first four terms of fit.py:149-152 at one-hot q.
 * out (G,) doubles. */
int fcd_gibbs_logjoint(fcd_ctx *ctx, const double *S_B, const double *lM, const double *hyper,
                       const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                       double *out, fcd_stream stream);
/* Number of anomalous (region, patient) sites of each chain, sum_{n,u} r_nu: out (G,) uint32 (overwritten).  The second
 * scalar of the chain diagnostics (split R-hat / ESS), next to the log-joint. */
int fcd_gibbs_chain_rsum(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, uint32_t *out,
                         fcd_stream stream);
/* Unnormalised conditional log-weights of EVERY site given the current state, nothing updated:
 * cond_f (G, C, 3), cond_r (G, Nreg, U, 2).  Either may be NULL.  (Parity hook + Rao-Blackwell use.) */
int fcd_gibbs_conditionals(fcd_ctx *ctx, const double *S_B, const double *lM, const double *hyper,
                           const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U,
                           int64_t G, int edge_mode, double *cond_f, double *cond_r, fcd_stream stream);
/* Plain views of the packed state: f (G, C) uint8, r (G, Nreg, U) uint8. */
int fcd_gibbs_export_state(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg,
                           int64_t U, int64_t G, uint8_t *f, uint8_t *r, fcd_stream stream);
/* ... and back (an r byte other than 0 is 1).  Every f byte must be 0, 1 or 2: the state another value makes is
 * undefined (the counting entry points may disagree on it).  The sampler itself never produces one. */
int fcd_gibbs_import_state(fcd_ctx *ctx, const uint8_t *f, const uint8_t *r, int64_t Nreg, int64_t U,
                           int64_t G, uint8_t *f_state, uint64_t *r_bits, fcd_stream stream);
/* 53-bit uniforms of the counter RNG for a list of (idx, chain, sweep, kind) counters:
 * out[2*i + half].  Lets a host binding check its own Philox against the device's. */
int fcd_philox_uniforms(fcd_ctx *ctx, const uint32_t *ctr4, int64_t n, uint64_t seed, double *out,
                        fcd_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* FCDIFF_HIP_H */
