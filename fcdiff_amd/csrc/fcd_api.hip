// Context, error strings and the host-side index maps of libfcdiff_hip.so.
#include <new>
#include <stdlib.h>

#include "fcd_common.h"
#include "fcd_fastmath.h"

#ifdef FCD_ABLATE
__device__ int fcd_abl_level[4];
__device__ unsigned long long *fcd_trace_buf;
void fcd_abl_refresh(hipStream_t s) {
    unsigned long long *tp = nullptr;
    if (const char *e = getenv("FCD_TRACE_PTR")) tp = (unsigned long long *)strtoull(e, nullptr, 0);
    (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(fcd_trace_buf), &tp, sizeof(tp), 0, hipMemcpyHostToDevice, s);
    int v[4] = {0, 0, 0, 0};
    if (const char *e = getenv("FCD_ABL_F")) v[0] = atoi(e);
    if (const char *e = getenv("FCD_ABL_PANEL")) v[1] = atoi(e);
    if (const char *e = getenv("FCD_ABL_DIAG")) v[2] = atoi(e);
    if (const char *e = getenv("FCD_TRACE_ROW")) v[3] = atoi(e);       // stamps inside one row of the pipelined scan
    (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(fcd_abl_level), v, sizeof(v), 0, hipMemcpyHostToDevice, s);
}
#endif

int fcd_buf_reserve(fcd_ctx *ctx, fcd_dev_buf &b, size_t bytes) {
    if (bytes <= b.bytes) return FCD_OK;
    // grow: the old block may still be in use by kernels already queued, so drain first
    FCD_HIP_TRY(hipDeviceSynchronize());
    void *old = b.p;
    b.p = nullptr;
    b.bytes = 0;
    if (old) FCD_HIP_TRY(hipFree(old));
    const size_t want = bytes < b.min_bytes ? b.min_bytes : bytes;
    void *p = nullptr;
    FCD_HIP_TRY(hipMalloc(&p, want));
    if (b.counted) ctx->n_alloc += 1;
    if (b.zeroed) {
        const hipError_t e = hipMemset(p, 0, want);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return (int)e;
        }
    }
    b.p = p;
    b.bytes = want;
    return FCD_OK;
}
// the grow-only blocks of a context, for what walks them all
static fcd_dev_buf fcd_ctx::*const ctx_bufs[] = {&fcd_ctx::ws,        &fcd_ctx::fsq,      &fcd_ctx::frec,
                                                 &fcd_ctx::noise_rec, &fcd_ctx::count_ws, &fcd_ctx::corr_tickets};

void fcd_prof_begin(fcd_ctx *ctx, int slot, hipStream_t s) {
    if (!ctx->prof_on) return;
    if (ctx->prof_n[slot] >= ctx->prof_cap[slot]) {
        const int cap = ctx->prof_cap[slot] ? ctx->prof_cap[slot] * 2 : 256;
        hipEvent_t *ev = new (std::nothrow) hipEvent_t[2 * cap];
        if (!ev) return;
        for (int i = 0; i < 2 * ctx->prof_cap[slot]; ++i) ev[i] = ctx->prof_ev[slot][i];
        for (int i = 2 * ctx->prof_cap[slot]; i < 2 * cap; ++i)
            if (hipEventCreate(&ev[i]) != hipSuccess) { delete[] ev; return; }
        delete[] ctx->prof_ev[slot];
        ctx->prof_ev[slot] = ev;
        ctx->prof_cap[slot] = cap;
    }
    (void)hipEventRecord(ctx->prof_ev[slot][2 * ctx->prof_n[slot]], s);
}

void fcd_prof_end(fcd_ctx *ctx, int slot, hipStream_t s) {
    if (!ctx->prof_on || ctx->prof_n[slot] >= ctx->prof_cap[slot]) return;
    (void)hipEventRecord(ctx->prof_ev[slot][2 * ctx->prof_n[slot] + 1], s);
    ctx->prof_n[slot] += 1;
}

extern "C" {

int fcd_prof_enable(fcd_ctx *ctx, int on) {
    if (!ctx) return FCD_ERR_ARG;
    ctx->prof_on = on ? 1 : 0;
    for (int i = 0; i < FCD_PROF_SLOTS; ++i) ctx->prof_n[i] = 0;
    return FCD_OK;
}

int fcd_prof_collect(fcd_ctx *ctx, int slot, double *total_ms, int64_t *count) {
    if (!ctx || slot < 0 || slot >= FCD_PROF_SLOTS || !total_ms || !count) return FCD_ERR_ARG;
    double tot = 0.0;
    for (int i = 0; i < ctx->prof_n[slot]; ++i) {
        FCD_HIP_TRY(hipEventSynchronize(ctx->prof_ev[slot][2 * i + 1]));
        float ms = 0.f;
        FCD_HIP_TRY(hipEventElapsedTime(&ms, ctx->prof_ev[slot][2 * i], ctx->prof_ev[slot][2 * i + 1]));
        tot += ms;
    }
    *total_ms = tot;
    *count = ctx->prof_n[slot];
    ctx->prof_n[slot] = 0;
    return FCD_OK;
}

int fcd_abi_version(void) { return FCD_ABI_VERSION; }

const char *fcd_strerror(int code) {
    switch (code) {
        case FCD_OK: return "ok";
        case FCD_ERR_ARG: return "invalid argument (null pointer or non-positive size)";
        case FCD_ERR_SHAPE: return "invalid shape (number of connections must be a triangular number, Nreg >= 2)";
        case FCD_ERR_UNSUPPORTED: return "shape outside what the gfx950 kernels are built for";
        case FCD_ERR_INDEX: return "reference edge id out of range";
        case FCD_ERR_DEVICE: return "a kernel abandoned a device-side wait; the chain state is unusable";
        case FCD_ERR_COMM: return "RCCL: library not found or a call failed";
        default: break;
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "unknown fcdiff_hip error";
}

const char *fcd_last_message(const fcd_ctx *ctx) { return ctx ? ctx->msg : ""; }

int fcd_ctx_create(fcd_ctx **out) {
    if (!out) return FCD_ERR_ARG;
    *out = nullptr;
    int dev = 0;
    FCD_HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    FCD_HIP_TRY(hipGetDeviceProperties(&prop, dev));
    fcd_ctx *ctx = new (std::nothrow) fcd_ctx();
    if (!ctx) return (int)hipErrorOutOfMemory;
    ctx->device = dev;
    ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // the only place the environment is read: defaults of the knobs (fcd_ctx_set_knob changes them later)
    fcd_knobs_from_env(ctx->knobs, [](const char *name) -> const char * { return getenv(name); });
    // tables of K_lik's exp and log (fcd_fastmath.h): 2^(-j/64) and {1/m_i, log m_i}, made with the host's libm
    struct { double exp_tab[FCD_EXP_CELLS]; fcd_log_cell log_tab[FCD_LOG_CELLS]; } tabs;
    fcd_fm_make_tables(tabs.exp_tab, tabs.log_tab, exp2, log);
    // a fixed-size device block, zero-filled
    auto zeroed = [&](void **p, size_t bytes) -> int {
        FCD_HIP_TRY(hipMalloc(p, bytes));
        ctx->n_alloc += 1;
        FCD_HIP_TRY(hipMemset(*p, 0, bytes));
        return FCD_OK;
    };
    int rc = fcd_ws_reserve(ctx, ctx->ws.min_bytes);
    if (rc == FCD_OK) rc = (int)hipHostMalloc((void **)&ctx->dev_err, sizeof(unsigned), hipHostMallocDefault);
    if (rc == FCD_OK) rc = (int)hipHostMalloc((void **)&ctx->hint, sizeof(fcd_hint_words), hipHostMallocDefault);
    if (rc == FCD_OK) {
        *ctx->dev_err = 0u;
        ctx->hint->f = 0u;      // (build numbers start at 1)
        ctx->hint->r = 0u;
        rc = (int)hipMalloc(&ctx->log_tab, sizeof(tabs));
        ctx->n_alloc += 1;
    }
    if (rc == FCD_OK) rc = (int)hipMemcpy(ctx->log_tab, &tabs, sizeof(tabs), hipMemcpyHostToDevice);
    if (rc == FCD_OK) rc = zeroed(&ctx->acc, FCD_ACC_BYTES);
    if (rc == FCD_OK) rc = zeroed(&ctx->f_slots, FCD_F_SLOTS_BYTES);
    if (rc == FCD_OK) rc = zeroed(&ctx->nan_slots, FCD_NAN_SLOTS_BYTES);
    if (rc == FCD_OK) rc = zeroed((void **)&ctx->words, sizeof(fcd_dev_words));
    if (rc) {
        fcd_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return FCD_OK;
}

int fcd_ctx_destroy(fcd_ctx *ctx) {
    if (!ctx) return FCD_OK;
    (void)fcd_comm_destroy(ctx);
    const hipError_t e = ctx->ws.p ? hipFree(ctx->ws.p) : hipSuccess;       // (the one result reported)
    ctx->ws.p = nullptr;
    for (auto b : ctx_bufs)
        if ((ctx->*b).p) (void)hipFree((ctx->*b).p);
    void *const dev[] = {ctx->pool_counts, ctx->log_tab, ctx->rs_dev, ctx->pg_dev, ctx->pt_dev,
                         ctx->acc,         ctx->f_slots, ctx->nan_slots, ctx->words};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    if (ctx->dev_err) (void)hipHostFree((void *)ctx->dev_err);
    if (ctx->hint) (void)hipHostFree((void *)ctx->hint);
    for (int i = 0; i < FCD_PROF_SLOTS; ++i) {
        for (int j = 0; j < 2 * ctx->prof_cap[i]; ++j) (void)hipEventDestroy(ctx->prof_ev[i][j]);
        delete[] ctx->prof_ev[i];
    }
    delete ctx;
    return (int)e;
}

int fcd_ctx_reserve(fcd_ctx *ctx, int64_t Nreg, int64_t U, int64_t G) {
    if (!ctx || Nreg < 2 || U < 1 || G < 1) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_ctx_reserve: bad argument");
    const int64_t GW = (G + 63) / 64;
    size_t need = (size_t)64 * GW * 64 * sizeof(double);        // log-joint partials
    const size_t en = (size_t)ctx->num_cu * 8 * 8 * sizeof(double);  // energy partials
    if (en > need) need = en;
    const fcd_sweep_plan pl = fcd_sweep_plan_for(ctx, Nreg, U, GW);    // f / r pass scratch and the square f copy
    if (pl.ws_bytes > need) need = pl.ws_bytes;
    int rc = fcd_ws_reserve(ctx, need);
    if (rc) return rc;
    rc = fcd_buf_reserve(ctx, ctx->fsq, pl.fsq_bytes);
    if (rc) return rc;
    // the f pass's record table: a sweep loop that finds none runs the kernel that builds its records per tile, so a
    // device without room for it is no error
    if (pl.frec_bytes && ctx->knobs.f_records != 1 && fcd_buf_reserve(ctx, ctx->frec, pl.frec_bytes) != FCD_OK) (void)hipGetLastError();
    return FCD_OK;
}

int fcd_ctx_set_knob(fcd_ctx *ctx, const char *name, double value) {
    if (!ctx || !name) return FCD_ERR_ARG;
    if (!fcd_knobs_set(ctx->knobs, name, value)) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_ctx_set_knob: unknown knob");
    return FCD_OK;
}

int fcd_ctx_check(fcd_ctx *ctx) {
    if (!ctx) return FCD_ERR_ARG;
    if (ctx->dev_err && *ctx->dev_err == FCD_DEV_ERR_HARM_SITE)
        return fcd_fail(ctx, FCD_ERR_DEVICE, "fcd_site_harmonize: a site id outside 0..B-1 reached the device");
    if (ctx->dev_err && *ctx->dev_err)
        return fcd_fail(ctx, FCD_ERR_DEVICE, "a device-side wait of the pipelined r pass was abandoned: the chain state is unusable");
    return FCD_OK;
}

int fcd_ctx_clear_error(fcd_ctx *ctx) {
    if (!ctx) return FCD_ERR_ARG;
    if (ctx->dev_err) *ctx->dev_err = 0u;
    // whatever an abandoned launch left in the context-owned accumulators / tickets (zero between launches by contract)
    if (ctx->acc) FCD_HIP_TRY(hipMemset(ctx->acc, 0, FCD_ACC_BYTES));
    if (ctx->f_slots) FCD_HIP_TRY(hipMemset(ctx->f_slots, 0, FCD_F_SLOTS_BYTES));
    if (ctx->nan_slots) FCD_HIP_TRY(hipMemset(ctx->nan_slots, 0, FCD_NAN_SLOTS_BYTES));
    for (auto b : ctx_bufs)
        if ((ctx->*b).zeroed && (ctx->*b).p) FCD_HIP_TRY(hipMemset((ctx->*b).p, 0, (ctx->*b).bytes));
    return FCD_OK;
}

int fcd_ctx_stat(const fcd_ctx *ctx, const char *name, int64_t *out) {
    if (!ctx || !name || !out) return FCD_ERR_ARG;
    if (!strcmp(name, "n_alloc")) *out = ctx->n_alloc;
    else if (!strcmp(name, "ws_bytes")) *out = (int64_t)ctx->ws.bytes;
    else if (!strcmp(name, "fsq_bytes")) *out = (int64_t)ctx->fsq.bytes;
    else if (!strcmp(name, "r_form_last")) *out = ctx->r_form_last;
    else if (!strcmp(name, "pack_launches")) *out = ctx->n_pack;
    else if (!strcmp(name, "tally_f_in_pack")) *out = ctx->n_pack_tally;
    else if (!strcmp(name, "tally_f_in_r")) *out = ctx->n_r_tally;
    else if (!strcmp(name, "tally_f_in_f")) *out = ctx->n_f_tally;
    else if (!strcmp(name, "tally_in_r_max_rounds")) *out = R_TALLY_MAX_ROUNDS;
    else if (!strcmp(name, "f_rec_passes")) *out = ctx->n_frec_pass;
    else if (!strcmp(name, "f_rec_builds")) *out = ctx->n_frec_build;
    else if (!strcmp(name, "f_rec_bytes")) *out = (int64_t)ctx->frec.bytes;
    else if (!strcmp(name, "f_rec_min_sweeps")) *out = F_REC_MIN_SWEEPS;
    else if (!strcmp(name, "f_sure_passes")) *out = ctx->n_fsure_pass;
    else if (!strcmp(name, "f_run_passes")) *out = ctx->n_frun_pass;
    else if (!strcmp(name, "r_sure_passes")) *out = ctx->n_rsure_pass;
    else if (!strcmp(name, "r_sure_builds")) *out = ctx->n_rsure_build;
    else if (!strcmp(name, "pipe_grid")) *out = ctx->pipe_grid;
    else if (!strcmp(name, "pipe_capacity")) *out = ctx->pipe_capacity;
    else if (!strcmp(name, "comm_world")) *out = ctx->comm ? ctx->comm_world : 0;
    else if (!strcmp(name, "dev_err")) *out = ctx->dev_err ? (int64_t)*ctx->dev_err : 0;
    else if (!strcmp(name, "f_repeats") || !strcmp(name, "r_exact_rows") || !strcmp(name, "f_sure_tiles") ||
             !strcmp(name, "f_sure_fallbacks") || !strcmp(name, "r_sure_sites") || !strcmp(name, "r_sure_exceptions")) {
        // event counters kept on the device (a synchronising read: diagnostics only)
        fcd_dev_words v;
        FCD_HIP_TRY(hipMemcpy(&v, ctx->words, sizeof(v), hipMemcpyDeviceToHost));
        *out = (int64_t)(!strcmp(name, "f_repeats")           ? v.f_repeats
                         : !strcmp(name, "r_exact_rows")      ? v.r_exact_rows
                         : !strcmp(name, "f_sure_tiles")      ? v.f_sure_tiles
                         : !strcmp(name, "f_sure_fallbacks")  ? v.f_sure_fallbacks
                         : !strcmp(name, "r_sure_sites")      ? v.r_sure_sites
                                                              : v.r_sure_exceptions);
    }
    else return FCD_ERR_ARG;
    return FCD_OK;
}

int64_t fcd_N_to_C(int64_t Nreg) { return fcd_tri(Nreg); }

int64_t fcd_C_to_N(int64_t C) {
    if (C < 1) return FCD_ERR_SHAPE;
    int64_t n = (int64_t)((sqrt(8.0 * (double)C + 1.0) - 1.0) * 0.5) + 1;
    while (fcd_tri(n) > C) --n;
    while (fcd_tri(n + 1) <= C) ++n;
    return fcd_tri(n) == C ? n : (int64_t)FCD_ERR_SHAPE;
}

int64_t fcd_nm_to_c(int64_t n, int64_t m) { return fcd_tri(n) + m; }

int fcd_c_to_nm(int64_t c, int64_t *n, int64_t *m) {
    if (c < 0 || !n || !m) return FCD_ERR_ARG;
    int nn, mm;
    fcd_edge_to_pair(c, nn, mm);
    *n = nn;
    *m = mm;
    return FCD_OK;
}

int64_t fcd_f_run_count(int64_t Nreg) { return Nreg < 2 ? (int64_t)FCD_ERR_SHAPE : fpr_runs((Nreg + 1) / 2); }

int fcd_f_run_locate(int64_t Nreg, int64_t t, int64_t *out9) {
    if (Nreg < 2 || Nreg > (1 << 20) || !out9 || t < 0 || t >= fpr_runs((Nreg + 1) / 2)) return FCD_ERR_ARG;
    const fpr_run R = fpr_locate((int)t, (int)Nreg);
    const int64_t v[9] = {R.n0, R.mb, R.cnt0, R.cnt1, R.tile0, R.ntile, R.cr0, R.cr1, fpr_philox_blocks(R)};
    for (int i = 0; i < 9; ++i) out9[i] = v[i];
    return FCD_OK;
}

}  // extern "C"
