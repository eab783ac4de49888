// Tuning / test knobs of a context: the fields, and ONE table that says for each its ABI name (fcd_ctx_set_knob), its member and
// the environment variable that sets its default, if any.  Plain C++, nothing from HIP: tests/ctx_check.cpp drives it under g++.
// The environment is read ONCE, by fcd_ctx_create through fcd_knobs_from_env; afterwards a knob changes only through
// fcd_ctx_set_knob: no entry point reads the environment.
#pragma once
#include <stdlib.h>
#include <string.h>

struct fcd_knobs {
    int r_path;        // 0: blocked r pass -- pipelined one-launch form where its grid fits the device at once, else one launch
                       // per block step; 3: one launch per block step always
    int r_ub;          // patients per panel workgroup of the blocked r pass: 0 = automatic, else 1 / 2 / 4
    int r_nopad;       // 1: no empty workgroups beside the in-order workgroups
    int r_refill;      // 1: the packing launch writes the panel-value sentinels in every sweep (default: only in the first sweep of a fcd_gibbs_run call)
    int qr_form;       // variational q_R update: 0 = by size; 1 = gathers from the edge-major table inside the region loop (rounds 1-3);
                       // 2 = region-major weights made first, whatever their size
    int r_coop;        // pipelined r pass: 1 = cooperative launch (the runtime checks that the grid is co-resident; +16 us per pass), else plain;
                       // 2 = TEST HOOK (fcd_ctx_set_knob only): every pipelined launch acts as if the runtime had refused it, launching nothing
    int r_dsplit;      // 1: ONE in-order workgroup per patient in the pipelined r pass (default: two, 8 chain words each, where there are more than 8)
    double r_tol;      // > default: widen the margin inside which an r draw is re-decided with the exact logit
    double f_tol;      // > default: the same for the f draws
    int r_poll_limit;  // TEST HOOK: > 0 bounds every device-side poll of the pipelined r pass by this many polls (default 2^20, ~1 s)
    int r_withhold;    // TEST HOOK: 1 = the in-order role of the pipelined r pass never sets its marks (a panel wave then gives up)
    int corr_form;     // 1: K_corr in 64 x 64 blocks with a moments pass also where the one-workgroup-per-subject kernel would run
    int f_form;        // 0: automatic; 2: the any-U pair kernel also where the U <= 64 one would run; 3: scalar-mask form
    int f_pack;        // 1: the r pass's packing launch in every sweep (default: only where the f pass cannot write the packed f words)
    int f_records;     // pair-tile f pass reads pair records made once per call: 0 = in calls of at least F_REC_MIN_SWEEPS pair-tile
                       // sweeps, 1 = never (every tile builds its own), 2 = whenever the pair-tile form runs
    int f_sure;        // 1: never the decided-tile path of the pair-tile f pass (A/B runs and tests; default: where the table has such tiles)
    int f_runs;        // form of the decided path: 0 = block-wide runs of tiles (gibbs_f_run_kernel) where the record build found EVERY
                       // tile decided, the per-tile kernel elsewhere; 1 = never the run form; 2 = the run form wherever the
                       // decided path is taken at all (tests: open edges inside the run kernel)
    int tally_in_r;    // f half of the tally inside the pipelined r pass (its in-order workgroups, before their first block): 0 = where
                       // a wave's rounds are at most R_TALLY_MAX_ROUNDS, 1 = never (the tally after the pass counts f), 2 = wherever
                       // the form allows (16-wave in-order workgroups)
    int tally_in_f;    // f half of the tally inside the f pass's run kernel (gibbs_f_run_kernel counts what it stores): 0 = where a
                       // sparse r pass follows in the same sweep (nothing else then carries it), 1 = never, 2 = wherever the run
                       // form runs (tests: ahead of the pipelined and the step form)
    int partial_chunk; // > 0: fcd_corr_partial walks at most this many subjects per chunk (tests: the chunking changes no bit)
    int tangent_chunk; // > 0: the same for fcd_tangent_fit and fcd_tangent_apply (subjects) and fcd_sym_eigh (matrices)
    int r_keep_words;  // 1: the tally makes the next pass's r words from the r bits (default: the pass's two r-word buffers swap
                       // roles from sweep to sweep -- what a pass wrote as r_Sn is the next pass's r_S)
    int r_sure;        // sparse r pass (gibbs_r_sparse_kernel: the sums of sites the tables decide are skipped): 0 = where the call's
                       // bound build finds at least R_SURE_MIN_SHARE of the sites decided, 1 = never, 2 = wherever the bounds exist
    double r_sure_x;   // TEST HOOK: > 1e-6 widens the range of x a decided site leaves to the full evaluation (0.25: half of all draws)
};

// One row per knob.  The ABI name is the member's name.  env == nullptr: through fcd_ctx_set_knob only, never from the
// environment (the test hooks, and what only A/B runs and tests set).
struct fcd_knob_row {
    const char *name;
    int fcd_knobs::*i;         // the member where it is an int (a value is truncated as (int)value) ...
    double fcd_knobs::*d;      // ... or where it is a double: exactly one of the two is set
    const char *env;
};
#define FCD_KNOB_I(m, env) {#m, &fcd_knobs::m, nullptr, env}
#define FCD_KNOB_D(m, env) {#m, nullptr, &fcd_knobs::m, env}
static const fcd_knob_row fcd_knob_table[] = {
    FCD_KNOB_I(r_path, "FCD_R_PATH"),
    FCD_KNOB_I(r_ub, "FCD_R_UB"),
    FCD_KNOB_I(r_nopad, "FCD_R_NOPAD"),
    FCD_KNOB_I(r_dsplit, "FCD_R_DSPLIT"),
    FCD_KNOB_I(r_coop, "FCD_R_COOP"),
    FCD_KNOB_I(qr_form, "FCD_QR_FORM"),
    FCD_KNOB_I(r_refill, "FCD_R_REFILL"),
    FCD_KNOB_D(r_tol, "FCD_R_TOL"),
    FCD_KNOB_D(f_tol, "FCD_F_TOL"),
    FCD_KNOB_I(f_form, "FCD_F_FORM"),
    FCD_KNOB_I(f_pack, "FCD_F_PACK"),
    FCD_KNOB_I(corr_form, "FCD_CORR_FORM"),
    FCD_KNOB_I(tally_in_r, "FCD_TALLY_IN_R"),
    FCD_KNOB_I(r_keep_words, "FCD_R_KEEP_WORDS"),
    FCD_KNOB_I(f_records, nullptr),
    FCD_KNOB_I(f_sure, nullptr),
    FCD_KNOB_I(f_runs, nullptr),
    FCD_KNOB_I(r_sure, nullptr),
    FCD_KNOB_D(r_sure_x, nullptr),
    FCD_KNOB_I(tally_in_f, nullptr),
    FCD_KNOB_I(partial_chunk, nullptr),
    FCD_KNOB_I(tangent_chunk, nullptr),
    FCD_KNOB_I(r_poll_limit, nullptr),
    FCD_KNOB_I(r_withhold, nullptr),
};
#undef FCD_KNOB_I
#undef FCD_KNOB_D
constexpr int FCD_KNOB_N = (int)(sizeof(fcd_knob_table) / sizeof(fcd_knob_table[0]));

// false: no knob of that name
static inline bool fcd_knobs_set(fcd_knobs &k, const char *name, double value) {
    for (const fcd_knob_row &r : fcd_knob_table) {
        if (strcmp(name, r.name)) continue;
        if (r.d) k.*r.d = value;
        else k.*r.i = (int)value;
        return true;
    }
    return false;
}

// The defaults: every knob 0, then the rows that name a variable from getenv_fn(name) -> const char * or nullptr.
// "0", "" and unset mean "default"; anything else is the number.
template <class GetEnv>
static inline void fcd_knobs_from_env(fcd_knobs &k, GetEnv getenv_fn) {
    k = fcd_knobs{};
    for (const fcd_knob_row &r : fcd_knob_table) {
        const char *e = r.env ? getenv_fn(r.env) : nullptr;
        if (e && *e) fcd_knobs_set(k, r.name, atof(e));
    }
    k.r_coop = k.r_coop == 1 ? 1 : 0;      // (2, the refusal test hook, not from the environment)
}
