// Repeated sessions per patient, with or without a known sampling variance per subject: the likelihood tables and the
// connection posterior for bt (C, U, K), K scans of each patient, session the fastest index (a 2-D bt is K = 1).
//
// F~_cu is the patient's latent state of the connection and the K sessions are conditionally independent measurements of
// it, so the density of an item given F~ = j is the product over its sessions:
//   P_j(c,u)  = prod_k N(bt[c,u,k]; mu_j, s_juk)                   (a NaN session contributes 1 under FCD_DATA_NAN_MISSING)
//   M_kl(c,u) = e_l P_k + (1 - e_l)/2 sum_{j != k} P_j             (e_l = _eval_M_eps, as in K_lik)
// A product of K densities underflows (sigma = 0.05, 16 sessions at 1.0: every P_j = 0 in fp64), so it is never formed:
//   a_j = sum_k ln N_j(x_k)  (ascending k, fp64),  m = max_j a_j,  p_j = exp(a_j - m),
//   lM  = m + ln M_kl(p).
// One p_j is exactly 1, so every M_kl(p) >= cmin > 0 and the nine logs take lik_logs' branch-free form (its general log
// where eps is 0 or 1).  A NaN session adds exactly 0.0 to a_j whatever its variance: the table of K sessions with one of
// them NaN everywhere equals the table of the other K - 1 bit for bit.  An item with no observed session is stored as 0.0
// by a select; m = -inf (every density of some session underflowed its log) gives -inf in all nine entries.
//
// Where a session's ln N_j comes from is the one thing the forms of a kernel differ in (the template parameter TERMS):
//   TERMS_SIGMA    the *_sessions entry points: s_juk = sigma_j, ln N_j = lik_normal_logs (a division by sigma_j).
//   TERMS_GLOBAL,  the *_noise entry points: a sampling variance per control (var_b[h]) and per patient session
//   TERMS_LDS      (var_bt[u*K + k]) on top of the population spread,
//                    b_ch | F_c = k ~ N(mu_k, sigma_k^2 + var_b[h]),   bt_cuk | F~_cu = j ~ N(mu_j, sigma_j^2 + var_bt[u,k]),
//                  ln N_j = -z*z/2 - (ln s_juk + ln sqrt(2 pi)),  z = (x - mu_j) * (1 / s_juk),  s_juk = sqrt(sigma_j^2 + var_bt[u,k]).
// The per-subject constants are made ONCE per call by noise_records_kernel, six doubles per subject-session -- 1/s_j and
// ln s_j + ln sqrt(2 pi), j = 0..2 -- into a block the context owns (fcd_ctx::noise_rec).  The item loops then do no fp64
// division, square root or logarithm per session: three multiplications by looked-up reciprocals where the sigma form
// divides.  Layout: pairs {1/s_j, ln s_j + ln sqrt(2 pi)} of 16 bytes, state-major inside a session, patient fastest,
//   bt records  rec[(k*3 + j)*U + u]     (double2)
//   b records   rec[j*H + h]
// so that the lanes of a wave, which hold consecutive patients (or consecutive h), read consecutive pairs: three 16-byte
// LDS reads per session, global reads coalesced.  Where max(H, U*K) <= NOISE_LDS_RECORDS (TERMS_LDS) every block copies the
// records of its role (item blocks the bt records, S_B blocks the b records) into dynamic LDS beside the stage buffer;
// above it (TERMS_GLOBAL) the loops read the same layout from global memory (it stays in L2: 48 bytes per
// subject-session).  A block that copies records takes at least one tile (one pass of the shared kernel) per
// NOISE_COPY_PER_TILE bytes of them, so the grid is smaller than the sigma form's where the records are many: at 400
// records every block would otherwise copy 19 KB to work on one tile of 16 KB.  Such a grid is held to the blocks
// resident at once.
//
// Four kernels:
//   lik_sessions_kernel         K_lik's launch: item blocks (one thread per (c,u), results through the LDS transpose and
//                               non-temporal 16-byte stores) and S_B blocks: lik_sb_block where there are no control
//                               variances (so S_B and lp_B_g_F equal fcd_lik_tables_ex's bit for bit), else the same block
//                               with s_kh = sqrt(sigma_k^2 + var_b[h]).  The K doubles of a tile's 256 items are one
//                               contiguous span of 256 K doubles: it is loaded coalesced through `stage` before the results
//                               overwrite it, at most 9 sessions per item and pass, so the kernel holds K_lik's LDS (and
//                               the records) and no more.
//   lik_shared_sessions_kernel  K_lik_shared's launch with the session-summed item: L[c] = sum_u lM[c,u], no per-patient
//                               table is written.
//   lik_grouped_kernel          the shared launch with the patient sum segmented by known groups of patients: L[c, g] (see
//                               the kernel).
//   posterior_sessions_kernel   fcd_post.hip's posterior_kernel with a_j summed over the item's sessions; an item with no
//                               observed session gets the prior law.
// The tuned 2-D kernels (lik_kernel, lik_shared_kernel, posterior_kernel) keep their own text and are not changed by this
// file: routed through shared helpers lik_kernel compiles to another schedule (fcd_lik_common.h).
#include "fcd_lik_common.h"

#define FCD_NOISE_LDS_RECORDS 768        // fcdiff_amd/tables.py: NOISE_LDS_RECORDS (the tests take both sides of it)

namespace {

constexpr int SESS_PASS = 9;             // sessions per item and pass: 256 x 9 doubles, the stage buffer of the results
constexpr int NOISE_LDS_RECORDS = FCD_NOISE_LDS_RECORDS;    // 768 x 48 B = 36 KiB beside 26.5 KiB of stage buffer and tables
constexpr int64_t NOISE_COPY_PER_TILE = 4096;               // bytes of records a block may copy per tile it takes

enum { TERMS_SIGMA, TERMS_GLOBAL, TERMS_LDS };              // the source of a session's terms: see the header

typedef double2 NoiseRec;                // {1 / s, ln s + ln sqrt(2 pi)}

// records of one call: the b records (3 H pairs, only where var_b is given), then the bt records (3 U K pairs)
__global__ __launch_bounds__(256) void noise_records_kernel(const double *__restrict__ var_b, const double *__restrict__ var_bt,
                                                            int H, int U, int K, LikTheta th, NoiseRec *__restrict__ rec_b,
                                                            NoiseRec *__restrict__ rec_bt) {
    const int64_t n_b = var_b ? (int64_t)H : 0, n_bt = (int64_t)U * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_b + n_bt; i += (int64_t)gridDim.x * blockDim.x) {
        double v;
        NoiseRec *r;
        int64_t stride;
        if (i < n_b) {
            v = var_b[i];
            r = rec_b + i;
            stride = H;
        } else {
            const int64_t q = i - n_b;               // u*K + k, the order of var_bt
            const int64_t u = q / K, k = q - u * K;
            v = var_bt ? var_bt[q] : 0.0;
            r = rec_bt + (k * 3) * (int64_t)U + u;
            stride = U;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double s = sqrt(th.sigma[j] * th.sigma[j] + v);
            r[j * stride] = make_double2(1.0 / s, log(s) + kLogSqrt2Pi);
        }
    }
}

// the record of patient u's session k for sess_add (nullptr: TERMS_SIGMA has none); rec_lds = the block's copy of rec_bt
template <int TERMS>
__device__ __forceinline__ const NoiseRec *sess_rec(const NoiseRec *__restrict__ rec_bt, const NoiseRec *rec_lds, int64_t k, int U,
                                                    unsigned u) {
    if (TERMS == TERMS_LDS) return rec_lds + ((int)k * 3) * U + (int)u;
    if (TERMS == TERMS_GLOBAL) return rec_bt + (k * 3) * (int64_t)U + u;
    return nullptr;
}

// one session's three ln N_j into a[]; r = the session's record (sess_rec), its states `stride` pairs apart.  MISSING: a
// NaN session adds exactly 0.0 and is counted
template <bool MISSING, int TERMS>
__device__ __forceinline__ void sess_add(double x, const LikTheta &th, const NoiseRec *r, int64_t stride, double a[3], int &n_obs,
                                         unsigned &n_nan) {
    double l[3];
    if (TERMS == TERMS_SIGMA) {
        lik_normal_logs(x, th, l[0], l[1], l[2]);
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const NoiseRec q = r[j * stride];
            const double z = (x - th.mu[j]) * q.x;
            l[j] = -(z * z) / 2.0 - q.y;
        }
    }
    if (MISSING) {
        const bool miss = __builtin_isnan(x);
#pragma unroll
        for (int j = 0; j < 3; ++j) l[j] = miss ? 0.0 : l[j];
        n_nan += miss;
        n_obs += !miss;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) a[j] += l[j];
}

// v[k*3+l] = m + ln M_kl(exp(a - m)); `empty`: no observed session, exactly 0.0
__device__ __forceinline__ void sess_logs(const double a[3], bool empty, const LikTheta &th, const double *etab,
                                          const fcd_log_cell *ltab, double v[9]) {
    const double m = fmax(a[0], fmax(a[1], a[2]));
    double p[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = fcd_exp_neg(m - a[j], etab);       // one of them exactly 1; NaN stays NaN
    lik_logs(p, th, ltab, v);
    const bool dead = m == -__builtin_inf();                               // (a - m would be NaN)
#pragma unroll
    for (int j = 0; j < 9; ++j) v[j] = empty ? 0.0 : (dead ? -__builtin_inf() : m + v[j]);
}

// lik_sb_block with s_kh = sqrt(sigma_k^2 + var_b[h]): rec = the b records [3][H]
template <bool MISSING, int TERMS>
__device__ __forceinline__ void noise_sb_block(unsigned sb_block, int tid, const double *__restrict__ b, int64_t C, int H,
                                               const LikTheta &th, const NoiseRec *rec, double *__restrict__ S_B,
                                               double *__restrict__ lpB, unsigned long long *__restrict__ nan_slots,
                                               int *blk_nan) {
    const int sub = tid & 15;
    const int64_t c = (int64_t)sb_block * 16 + (tid >> 4);
    double s[3] = {0.0, 0.0, 0.0};
    int nan_b = 0;
    if (MISSING && tid == 0) *blk_nan = 0;
    if (c < C) {
        const double *row = b + c * H;
        for (int h = sub; h < H; h += 16) {
            const double x = row[h];
            double l[3] = {0.0, 0.0, 0.0};
            int n_obs = 0;
            unsigned n_nan = 0;
            sess_add<MISSING, TERMS>(x, th, rec + h, H, l, n_obs, n_nan);
            nan_b += (int)n_nan;
            if (lpB) {
                double *o = lpB + (c * H + h) * 3;
                o[0] = l[0]; o[1] = l[1]; o[2] = l[2];
            }
            s[0] += l[0]; s[1] += l[1]; s[2] += l[2];
        }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) s[j] += __shfl_xor(s[j], o, 16);
    }
    if (c < C && sub == 0) {
        S_B[c * 3 + 0] = s[0];
        S_B[c * 3 + 1] = s[1];
        S_B[c * 3 + 2] = s[2];
    }
    if (MISSING) {
        __syncthreads();
        if (nan_b) atomicAdd(blk_nan, nan_b);
        __syncthreads();
        if (tid == 0 && *blk_nan && nan_slots)
            atomicAdd(&nan_slots[(blockIdx.x % FCD_NAN_SLOTS) * 16 + 0], (unsigned long long)*blk_nan);
    }
}

// the S_B blocks of both table kernels; no control variances (TERMS_SIGMA, or rec_b == nullptr): K_lik's own block
template <bool MISSING, int TERMS>
__device__ __forceinline__ void sess_sb_role(unsigned sb_block, int tid, const double *__restrict__ b, int64_t C, int H,
                                             const LikTheta &th, const NoiseRec *__restrict__ rec_b, NoiseRec *rec_lds,
                                             double *__restrict__ S_B, double *__restrict__ lpB,
                                             unsigned long long *__restrict__ nan_slots, int *blk_nan) {
    if (TERMS == TERMS_SIGMA || !rec_b) {
        lik_sb_block<MISSING>(sb_block, tid, b, C, H, th, S_B, lpB, nan_slots, blk_nan);
    } else if (TERMS == TERMS_LDS) {
        for (int t = tid; t < 3 * H; t += LIK_BLOCK) rec_lds[t] = rec_b[t];      // (H <= NOISE_LDS_RECORDS)
        __syncthreads();
        noise_sb_block<MISSING, TERMS>(sb_block, tid, b, C, H, th, rec_lds, S_B, lpB, nan_slots, blk_nan);
    } else {
        noise_sb_block<MISSING, TERMS>(sb_block, tid, b, C, H, th, rec_b, S_B, lpB, nan_slots, blk_nan);
    }
}

template <bool MISSING, int TERMS>
__global__ __launch_bounds__(LIK_BLOCK) void lik_sessions_kernel(const double *__restrict__ bt, int64_t n_items, int U, int K,
                                                                 LikTheta th, const LikTabs *__restrict__ tabs,
                                                                 const NoiseRec *__restrict__ rec_b,
                                                                 const NoiseRec *__restrict__ rec_bt,
                                                                 double *__restrict__ lM, int n_bt_blocks,
                                                                 const double *__restrict__ b, int64_t C, int H,
                                                                 double *__restrict__ S_B, double *__restrict__ lpB,
                                                                 unsigned long long *__restrict__ nan_slots) {
    __shared__ __attribute__((aligned(16))) double stage[LIK_BLOCK * SESS_PASS];
    __shared__ __attribute__((aligned(16))) fcd_log_cell ltab[FCD_LOG_CELLS];
    __shared__ double etab[FCD_EXP_CELLS];
    __shared__ int blk_nan;
    extern __shared__ __attribute__((aligned(16))) NoiseRec rec_lds[];      // TERMS_LDS: 3 max(H, U K) pairs; else unused
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_bt_blocks) {
        sess_sb_role<MISSING, TERMS>(blockIdx.x - n_bt_blocks, tid, b, C, H, th, rec_b, rec_lds, S_B, lpB, nan_slots, &blk_nan);
        return;
    }
    for (int t = tid; t < FCD_LOG_CELLS; t += LIK_BLOCK) ltab[t] = tabs->log_tab[t];
    if (tid < FCD_EXP_CELLS) etab[tid] = tabs->exp_tab[tid];
    if (TERMS == TERMS_LDS)
        for (int t = tid; t < 3 * U * K; t += LIK_BLOCK) rec_lds[t] = rec_bt[t];   // (U K <= NOISE_LDS_RECORDS)
    if (MISSING && tid == 0) blk_nan = 0;
    __syncthreads();
    unsigned n_nan = 0;
    const int64_t n_tiles = (n_items + LIK_BLOCK - 1) / LIK_BLOCK;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += n_bt_blocks) {
        const int64_t base = tile * LIK_BLOCK;
        const int n_here = (n_items - base < LIK_BLOCK) ? (int)(n_items - base) : LIK_BLOCK;
        const unsigned u = (unsigned)((unsigned)(base % U) + (unsigned)tid) % (unsigned)U;     // the item's patient (sess_rec)
        double a[3] = {0.0, 0.0, 0.0};
        int n_obs = 0;
        for (int64_t k0 = 0; k0 < K; k0 += SESS_PASS) {
            const int P = (K - k0 < SESS_PASS) ? (int)(K - k0) : SESS_PASS;
#ifdef FCD_SESS_STRIDED
            // measurement build only (profiles/sessions_cost.py): every thread reads its own item's sessions, K doubles apart
            if (tid < n_here) {
                const double *x = bt + (base + tid) * K + k0;
                for (int s = 0; s < P; ++s)
                    sess_add<MISSING, TERMS>(x[s], th, sess_rec<TERMS>(rec_bt, rec_lds, k0 + s, U, u), U, a, n_obs, n_nan);
            }
#else
            const int n = n_here * P;                               // <= 256 * 9: the pass fits the stage buffer
            const double *src = bt + base * K + k0;                 // item q's sessions k0 .. k0 + P - 1 at src + q K
            if (P == K) {
                for (int j = tid; j < n; j += LIK_BLOCK) stage[j] = src[j];           // (rows of odd K are 8-byte aligned)
            } else {
                for (int j = tid; j < n; j += LIK_BLOCK) {
                    const int q = j / P;
                    stage[j] = src[(int64_t)q * K + (j - q * P)];
                }
            }
            __syncthreads();
            if (tid < n_here)
                for (int s = 0; s < P; ++s)
                    sess_add<MISSING, TERMS>(stage[tid * P + s], th, sess_rec<TERMS>(rec_bt, rec_lds, k0 + s, U, u), U, a, n_obs,
                                             n_nan);
            __syncthreads();                                        // the pass is read: the next one, or the results
#endif
        }
        if (tid < n_here) {
            double v[9];
            sess_logs(a, MISSING && n_obs == 0, th, etab, ltab, v);
#pragma unroll
            for (int j = 0; j < 9; ++j) stage[tid * 9 + j] = v[j];
        }
        __syncthreads();
        const int64_t n_dbl = (int64_t)n_here * 9;
        double *dst = lM + base * 9;
        // base*9*8 bytes is a multiple of 16 (LIK_BLOCK*72), so double2 stores are aligned; non-temporal as in lik_kernel
        const int64_t n_d2 = n_dbl >> 1;
        const double2 *s2 = reinterpret_cast<const double2 *>(stage);
        double2 *d2 = reinterpret_cast<double2 *>(dst);
        {
            typedef double d2v __attribute__((ext_vector_type(2)));
            for (int64_t j = tid; j < n_d2; j += LIK_BLOCK)
                __builtin_nontemporal_store(*reinterpret_cast<const d2v *>(&s2[j]), reinterpret_cast<d2v *>(&d2[j]));
        }
        if ((n_dbl & 1) && tid == 0) dst[n_dbl - 1] = stage[n_dbl - 1];
        __syncthreads();
    }
    if (MISSING) {
        if (n_nan) atomicAdd(&blk_nan, (int)n_nan);
        __syncthreads();
        if (tid == 0 && blk_nan && nan_slots)
            atomicAdd(&nan_slots[(blockIdx.x % FCD_NAN_SLOTS) * 16 + 1], (unsigned long long)blk_nan);
    }
}

template <bool MISSING, int TERMS, int G>
__global__ __launch_bounds__(LIK_BLOCK) void lik_shared_sessions_kernel(const double *__restrict__ bt, int64_t C, int U, int K,
                                                                        LikTheta th, const LikTabs *__restrict__ tabs,
                                                                        const NoiseRec *__restrict__ rec_b,
                                                                        const NoiseRec *__restrict__ rec_bt,
                                                                        double *__restrict__ L, int n_l_blocks,
                                                                        const double *__restrict__ b, int H,
                                                                        double *__restrict__ S_B,
                                                                        unsigned long long *__restrict__ nan_slots) {
    static_assert(G == 16 || G == 32 || G == 64, "lane group of 16, 32 or 64");
    __shared__ __attribute__((aligned(16))) fcd_log_cell ltab[FCD_LOG_CELLS];
    __shared__ double etab[FCD_EXP_CELLS];
    __shared__ int blk_nan;
    extern __shared__ __attribute__((aligned(16))) NoiseRec rec_lds[];      // TERMS_LDS: 3 max(H, U K) pairs; else unused
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_l_blocks) {
        sess_sb_role<MISSING, TERMS>(blockIdx.x - n_l_blocks, tid, b, C, H, th, rec_b, rec_lds, S_B, nullptr, nan_slots, &blk_nan);
        return;
    }
    for (int t = tid; t < FCD_LOG_CELLS; t += LIK_BLOCK) ltab[t] = tabs->log_tab[t];
    if (tid < FCD_EXP_CELLS) etab[tid] = tabs->exp_tab[tid];
    if (TERMS == TERMS_LDS)
        for (int t = tid; t < 3 * U * K; t += LIK_BLOCK) rec_lds[t] = rec_bt[t];   // (U K <= NOISE_LDS_RECORDS)
    if (MISSING && tid == 0) blk_nan = 0;
    __syncthreads();
    constexpr int EPB = LIK_BLOCK / G;          // edges per block and pass
    const int lane = tid & (G - 1);
    unsigned n_nan = 0;
    for (int64_t c0 = (int64_t)blockIdx.x * EPB; c0 < C; c0 += (int64_t)n_l_blocks * EPB) {
        const int64_t c = c0 + tid / G;         // the same for the G lanes of a group
        double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (c < C) {
            for (int u = lane; u < U; u += G) {
                const double *x = bt + (c * U + u) * K;             // the item's K sessions
                double a[3] = {0.0, 0.0, 0.0}, v[9];
                int n_obs = 0;
                for (int k = 0; k < K; ++k)
                    sess_add<MISSING, TERMS>(x[k], th, sess_rec<TERMS>(rec_bt, rec_lds, k, U, u), U, a, n_obs, n_nan);
                sess_logs(a, MISSING && n_obs == 0, th, etab, ltab, v);
#pragma unroll
                for (int j = 0; j < 9; ++j) s[j] += v[j];
            }
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1)
#pragma unroll
            for (int j = 0; j < 9; ++j) s[j] += __shfl_xor(s[j], o, G);
        if (c < C && lane == 0) {
#pragma unroll
            for (int j = 0; j < 9; ++j) L[c * 9 + j] = s[j];
        }
    }
    if (MISSING) {
        __syncthreads();
        if (n_nan) atomicAdd(&blk_nan, (int)n_nan);
        __syncthreads();
        if (tid == 0 && blk_nan && nan_slots)
            atomicAdd(&nan_slots[(blockIdx.x % FCD_NAN_SLOTS) * 16 + 1], (unsigned long long)blk_nan);
    }
}

// The grouped tables (fcdiff_amd.fit.GroupedRegionFit): L[c, g] = sum over the members u of group g of lM[c, u], the patient
// sum of lik_shared_sessions_kernel segmented by KNOWN groups.  order (U,) lists the patients sorted by group, offsets (G + 1,)
// each group's span in it.  A lane group of W = 16, 32 or 64 lanes serves one (edge, group) pair and the grid strides over
// the C G pairs; lane i takes the members order[offsets[g] + i], + W, ... from the contiguous row bt[c, :], nine running sums
// per lane, a butterfly of shuffles, and lane 0 writes the 72-byte record at (c G + g) 9: no atomics in the sums, so two calls
// agree bit for bit.  W follows the shared kernels' rule (<= 16, <= 32, else 64) on the LARGEST group, which every block
// reads off `offsets` itself (G + 1 words from L2): the index arrays stay on the device and the host needs no copy of them.
// One group is therefore lik_shared_sessions_kernel statement for statement, and singletons give the unshared items' nine
// values unchanged (a one-term sum and a butterfly of zeros).  A member index outside [0, U) is skipped, never read.
template <bool MISSING, int TERMS, int W>
__device__ __forceinline__ void grouped_pairs(const double *__restrict__ bt, int64_t C, int U, int K, const LikTheta &th,
                                              const double *etab, const fcd_log_cell *ltab, const NoiseRec *__restrict__ rec_bt,
                                              const NoiseRec *rec_lds, const int32_t *__restrict__ order,
                                              const int64_t *__restrict__ offsets, int G, double *__restrict__ L, int n_l_blocks,
                                              unsigned &n_nan) {
    constexpr int PPB = LIK_BLOCK / W;          // pairs per block and pass
    const int tid = threadIdx.x;
    const int lane = tid & (W - 1);
    const int64_t n_pairs = C * G;
    for (int64_t p0 = (int64_t)blockIdx.x * PPB; p0 < n_pairs; p0 += (int64_t)n_l_blocks * PPB) {
        const int64_t p = p0 + tid / W;         // the same for the W lanes of a group
        double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (p < n_pairs) {
            const int64_t c = p / G;
            const int g = (int)(p - c * G);
            int64_t lo = offsets[g], hi = offsets[g + 1];
            lo = lo < 0 ? 0 : lo;
            hi = hi > U ? U : hi;
            const double *row = bt + c * U * K;                     // the edge's U K doubles: the gather stays inside them
            for (int64_t i = lo + lane; i < hi; i += W) {
                const unsigned u = (unsigned)order[i];
                if (u >= (unsigned)U) continue;
                const double *x = row + (int64_t)u * K;             // the item's K sessions
                double a[3] = {0.0, 0.0, 0.0}, v[9];
                int n_obs = 0;
                for (int k = 0; k < K; ++k)
                    sess_add<MISSING, TERMS>(x[k], th, sess_rec<TERMS>(rec_bt, rec_lds, k, U, u), U, a, n_obs, n_nan);
                sess_logs(a, MISSING && n_obs == 0, th, etab, ltab, v);
#pragma unroll
                for (int j = 0; j < 9; ++j) s[j] += v[j];
            }
        }
#pragma unroll
        for (int o = W / 2; o > 0; o >>= 1)
#pragma unroll
            for (int j = 0; j < 9; ++j) s[j] += __shfl_xor(s[j], o, W);
        if (p < n_pairs && lane == 0) {
#pragma unroll
            for (int j = 0; j < 9; ++j) L[p * 9 + j] = s[j];
        }
    }
}

template <bool MISSING, int TERMS>
__global__ __launch_bounds__(LIK_BLOCK) void lik_grouped_kernel(const double *__restrict__ bt, int64_t C, int U, int K, LikTheta th,
                                                                const LikTabs *__restrict__ tabs,
                                                                const NoiseRec *__restrict__ rec_b,
                                                                const NoiseRec *__restrict__ rec_bt,
                                                                const int32_t *__restrict__ order,
                                                                const int64_t *__restrict__ offsets, int G,
                                                                double *__restrict__ L, int n_l_blocks,
                                                                const double *__restrict__ b, int H, double *__restrict__ S_B,
                                                                unsigned long long *__restrict__ nan_slots) {
    __shared__ __attribute__((aligned(16))) fcd_log_cell ltab[FCD_LOG_CELLS];
    __shared__ double etab[FCD_EXP_CELLS];
    __shared__ int blk_nan;
    __shared__ int largest;                                                 // members of the largest group
    extern __shared__ __attribute__((aligned(16))) NoiseRec rec_lds[];      // TERMS_LDS: 3 max(H, U K) pairs; else unused
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_l_blocks) {
        sess_sb_role<MISSING, TERMS>(blockIdx.x - n_l_blocks, tid, b, C, H, th, rec_b, rec_lds, S_B, nullptr, nan_slots, &blk_nan);
        return;
    }
    for (int t = tid; t < FCD_LOG_CELLS; t += LIK_BLOCK) ltab[t] = tabs->log_tab[t];
    if (tid < FCD_EXP_CELLS) etab[tid] = tabs->exp_tab[tid];
    if (TERMS == TERMS_LDS)
        for (int t = tid; t < 3 * U * K; t += LIK_BLOCK) rec_lds[t] = rec_bt[t];   // (U K <= NOISE_LDS_RECORDS)
    if (tid == 0) {
        blk_nan = 0;
        largest = 0;
    }
    __syncthreads();
    {
        int64_t mine = 0;
        for (int g = tid; g < G; g += LIK_BLOCK) {
            const int64_t n = offsets[g + 1] - offsets[g];
            mine = n > mine ? n : mine;
        }
        if (mine > 0) atomicMax(&largest, mine > U ? U : (int)mine);
    }
    __syncthreads();
    const int big = largest;
    unsigned n_nan = 0;
    if (big <= 16)
        grouped_pairs<MISSING, TERMS, 16>(bt, C, U, K, th, etab, ltab, rec_bt, rec_lds, order, offsets, G, L, n_l_blocks, n_nan);
    else if (big <= 32)
        grouped_pairs<MISSING, TERMS, 32>(bt, C, U, K, th, etab, ltab, rec_bt, rec_lds, order, offsets, G, L, n_l_blocks, n_nan);
    else
        grouped_pairs<MISSING, TERMS, 64>(bt, C, U, K, th, etab, ltab, rec_bt, rec_lds, order, offsets, G, L, n_l_blocks, n_nan);
    if (MISSING) {
        __syncthreads();
        if (n_nan) atomicAdd(&blk_nan, (int)n_nan);
        __syncthreads();
        if (tid == 0 && blk_nan && nan_slots)
            atomicAdd(&nan_slots[(blockIdx.x % FCD_NAN_SLOTS) * 16 + 1], (unsigned long long)blk_nan);
    }
}

struct SessPostTheta {
    double mu[3], sigma[3], lsigma[3];      // (sigma and lsigma: TERMS_SIGMA only)
    double eps;           // epsilon
    double e[3];          // _eval_M_eps(eta, epsilon, l)
    double pT[3];         // p(T = 1 | l) = 0, 1, eta
};

// posterior_kernel (fcd_post.hip) statement for statement, except that a_j is summed over the item's K sessions before the
// maximum is taken.  MISSING: a NaN session is skipped; an item with no observed session takes N_j = 1, the prior law.
// TERMS_GLOBAL (there is no TERMS_LDS form): ln N_j of a session comes from the record of (u, k), with z through the
// record's reciprocal and the constant ln sqrt(2 pi), which is common to the three j of a session and leaves the law as it is.
template <bool MISSING, int TERMS>
__global__ __launch_bounds__(256) void posterior_sessions_kernel(const double *__restrict__ bt, int64_t C, int U, int K,
                                                                 SessPostTheta th, const NoiseRec *__restrict__ rec_bt,
                                                                 const uint32_t *__restrict__ counts,
                                                                 const double *__restrict__ lq_F, const double *__restrict__ lq_R,
                                                                 double *__restrict__ p_T, double *__restrict__ p_Ft,
                                                                 double *__restrict__ p_ch) {
    const int64_t items = C * U;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        double W[9];
        // the item's edge and patient, for the weights from lq_R and for the records; the sigma form with counts needs
        // neither.  (Made unconditionally, the sigma form spilt more SGPRs into lanes and measured 1 % slower.)
        const bool need_cu = TERMS != TERMS_SIGMA || !counts;
        const int64_t c = need_cu ? i / U : 0;
        const int u = need_cu ? (int)(i - c * U) : 0;
        if (counts) {
            const uint32_t *cw = counts + i * 9;
#pragma unroll
            for (int j = 0; j < 9; ++j) W[j] = (double)cw[j];
        } else {
            int n, m;
            fcd_edge_to_pair(c, n, m);
            const double q0n = exp(lq_R[((int64_t)n * U + u) * 2]), q1n = exp(lq_R[((int64_t)n * U + u) * 2 + 1]);
            const double q0m = exp(lq_R[((int64_t)m * U + u) * 2]), q1m = exp(lq_R[((int64_t)m * U + u) * 2 + 1]);
            double w[3];
            w[0] = q0n * q0m;
            w[1] = q1n * q1m;
            w[2] = q0n * q1m;
            w[2] += q1n * q0m;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double qF = exp(lq_F[c * 3 + k]);
#pragma unroll
                for (int l = 0; l < 3; ++l) W[k * 3 + l] = qF * w[l];
            }
        }
        const double *x = bt + i * K;
        double a[3] = {0.0, 0.0, 0.0};
        int n_obs = 0;
        for (int k = 0; k < K; ++k) {
            const double xk = x[k];
            if (MISSING && __builtin_isnan(xk)) continue;          // unobserved: the session's densities integrate to 1
            ++n_obs;
            if (TERMS == TERMS_SIGMA) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double z = (xk - th.mu[j]) / th.sigma[j];
                    a[j] += -(z * z) / 2.0 - th.lsigma[j];           // ln N_j up to the common ln sqrt(2 pi)
                }
            } else {
                const NoiseRec *r = rec_bt + ((int64_t)k * 3) * U + u;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const NoiseRec q = r[(int64_t)j * U];
                    const double z = (xk - th.mu[j]) * q.x;
                    a[j] += -(z * z) / 2.0 - q.y;
                }
            }
        }
        double N[3];
        if (MISSING && n_obs == 0) {
            N[0] = N[1] = N[2] = 1.0;
        } else {
            const double mx = fmax(a[0], fmax(a[1], a[2]));
#pragma unroll
            for (int j = 0; j < 3; ++j) N[j] = exp(a[j] - mx);
        }
        const double S[3] = {N[1] + N[2], N[0] + N[2], N[0] + N[1]};
        double wsum = 0.0, t1 = 0.0, ch = 0.0, ft[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                const double wt = W[k * 3 + l];
                if (wt == 0.0) continue;
                const double off = (1 - th.e[l]) * 0.5;
                const double M = th.e[l] * N[k] + off * S[k];
                if (!(M > 0.0)) continue;                    // (only at epsilon in {0, 1}: a case the model gives no mass)
                const double r = wt / M;
                wsum += wt;
                if (th.pT[l] != 0.0) t1 += th.pT[l] * (th.eps * N[k] + (1 - th.eps) * 0.5 * S[k]) * r;
                ch += off * S[k] * r;
#pragma unroll
                for (int j = 0; j < 3; ++j) ft[j] += ((j == k) ? th.e[l] : off) * N[j] * r;
            }
        }
        const double inv = 1.0 / wsum;
        p_T[i] = t1 * inv;
        p_ch[i] = ch * inv;
#pragma unroll
        for (int j = 0; j < 3; ++j) p_Ft[i * 3 + j] = ft[j] * inv;
    }
}

// ---------------------------------------------------------------------------------------------
// host

// the checks the table entry points share with their 2-D siblings; who = "sessions tables" or "noise tables".  `records`:
// the record forms, whose kernels index the U K records of a state with 32 bits
int sess_check(fcd_ctx *ctx, const char *who, bool records, int64_t C, int64_t H, int64_t U, int64_t K, int flags, bool counted) {
    if (flags & ~FCD_DATA_NAN_MISSING) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "unknown flags 0x%x", flags);
    if (counted && !(flags & FCD_DATA_NAN_MISSING))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "missing counts need FCD_DATA_NAN_MISSING");
    if (C < 1 || H < 1 || U < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "C=%lld and U=%lld (and H) must be >= 1", C, U);
    if (K < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "K=%lld sessions, must be >= 1", K);
    if (fcd_C_to_N(C) < 0) return fcd_fail(ctx, FCD_ERR_SHAPE, "Number of connections (%lld) must be a triangular number.", C);
    if (H > INT32_MAX || U > INT32_MAX || K > INT32_MAX || C * U > INT64_MAX / 8 / K || (records && U * K > ((int64_t)1 << 31)))
        return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "H/U/K too large");
    return FCD_OK;
}

// the records of one call, in the context's block: *rec_b (nullptr without var_b) and *rec_bt
int noise_records(fcd_ctx *ctx, const double *var_b, const double *var_bt, int64_t H, int64_t U, int64_t K, const LikTheta &th,
                  hipStream_t s, const NoiseRec **rec_b, const NoiseRec **rec_bt) {
    const int64_t n_b = var_b ? H : 0, n = n_b + U * K;
    int rc = fcd_buf_reserve(ctx, ctx->noise_rec, (size_t)n * 3 * sizeof(NoiseRec));
    if (rc) return rc;
    NoiseRec *base = static_cast<NoiseRec *>(ctx->noise_rec.p);
    *rec_b = var_b ? base : nullptr;
    *rec_bt = base + 3 * n_b;
    int64_t blocks = (n + 255) / 256;
    if (blocks > (int64_t)ctx->num_cu * 8) blocks = (int64_t)ctx->num_cu * 8;
    hipLaunchKernelGGL(noise_records_kernel, dim3((unsigned)blocks), dim3(256), 0, s, var_b, var_bt, (int)H, (int)U, (int)K, th,
                       base, base + 3 * n_b);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

// tiles (passes) a block takes at least: one per NOISE_COPY_PER_TILE bytes of records it copies into LDS
int64_t noise_tiles_per_block(size_t lds_record_bytes) {
    const int64_t t = ((int64_t)lds_record_bytes + NOISE_COPY_PER_TILE - 1) / NOISE_COPY_PER_TILE;
    return t < 1 ? 1 : t;
}

// what a table launch needs to know of its terms; the default is the sigma form's
struct SessTerms {
    int terms = TERMS_SIGMA;
    const NoiseRec *rec_b = nullptr, *rec_bt = nullptr;
    size_t lds = 0;               // dynamic LDS: the records of the larger role
    int64_t per_block = 1;        // tiles (passes) an item block takes at least
};

// the record form of a table call: makes the records and decides where the kernels read them
int noise_terms(fcd_ctx *ctx, const double *var_b, const double *var_bt, int64_t H, int64_t U, int64_t K, const LikTheta &th,
                hipStream_t s, SessTerms &t) {
    int rc = noise_records(ctx, var_b, var_bt, H, U, K, th, s, &t.rec_b, &t.rec_bt);
    if (rc) return rc;
    const int64_t n_rec = (t.rec_b && H > U * K) ? H : U * K;
    const bool in_lds = n_rec <= NOISE_LDS_RECORDS;
    t.terms = in_lds ? TERMS_LDS : TERMS_GLOBAL;
    t.lds = in_lds ? (size_t)n_rec * 3 * sizeof(NoiseRec) : 0;
    t.per_block = noise_tiles_per_block(in_lds ? (size_t)U * K * 3 * sizeof(NoiseRec) : 0);
    return FCD_OK;
}

// the instantiation of a table kernel that a call launches (and whose occupancy it asks for)
template <bool MISSING>
auto lik_sessions_fn(int terms) {
    return terms == TERMS_SIGMA    ? lik_sessions_kernel<MISSING, TERMS_SIGMA>
           : terms == TERMS_GLOBAL ? lik_sessions_kernel<MISSING, TERMS_GLOBAL>
                                   : lik_sessions_kernel<MISSING, TERMS_LDS>;
}

template <bool MISSING, int TERMS>
auto lik_shared_group_fn(int group) {
    return group == 16   ? lik_shared_sessions_kernel<MISSING, TERMS, 16>
           : group == 32 ? lik_shared_sessions_kernel<MISSING, TERMS, 32>
                         : lik_shared_sessions_kernel<MISSING, TERMS, 64>;
}

template <bool MISSING>
auto lik_shared_sessions_fn(int terms, int group) {
    return terms == TERMS_SIGMA    ? lik_shared_group_fn<MISSING, TERMS_SIGMA>(group)
           : terms == TERMS_GLOBAL ? lik_shared_group_fn<MISSING, TERMS_GLOBAL>(group)
                                   : lik_shared_group_fn<MISSING, TERMS_LDS>(group);
}

// n_missing2 = the sums of the NaN-count slots a table kernel has filled
int sess_nan_fold(unsigned long long *slots, int64_t *n_missing2, hipStream_t s) {
    if (slots) {
        hipLaunchKernelGGL(nan_fold_kernel, dim3(1), dim3(FCD_NAN_SLOTS), 0, s, slots, n_missing2);
        FCD_LAUNCH_CHECK();
    }
    return FCD_OK;
}

// the unshared tables: K_lik's grid (item blocks, then the S_B blocks) with the terms of `t`
int lik_sessions_launch(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U, int64_t K,
                        const LikTheta &th, const SessTerms &t, double *S_B, double *lM, double *lp_B_g_F, int flags,
                        int64_t *n_missing2, hipStream_t s) {
    const auto kernel = (flags & FCD_DATA_NAN_MISSING) ? lik_sessions_fn<true>(t.terms) : lik_sessions_fn<false>(t.terms);
    const int64_t n_items = C * U;
    const int64_t n_tiles = (n_items + LIK_BLOCK - 1) / LIK_BLOCK;
    int64_t grid = (n_tiles + t.per_block - 1) / t.per_block;
    int64_t cap = (int64_t)ctx->num_cu * 16;         // K_lik's measured choice: 16 blocks per CU, grid-stride beyond
    if (t.per_block > 1) {
        // blocks of several tiles: no more of them than are resident at once, or the few left over start when the others
        // are done and double the time (measured at K = 8: 778 blocks of 5 tiles on 768 places)
        int per_cu = 0;
        FCD_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(kernel), LIK_BLOCK, t.lds));
        if (per_cu >= 1 && (int64_t)ctx->num_cu * per_cu < cap) cap = (int64_t)ctx->num_cu * per_cu;
    }
    if (grid > cap) grid = cap;
    const int64_t n_b_blocks = (C + 15) / 16;
    // (counts are refused without FCD_DATA_NAN_MISSING: the forms that do not count get no slots)
    unsigned long long *slots = n_missing2 ? reinterpret_cast<unsigned long long *>(ctx->nan_slots) : nullptr;
    const LikTabs *tabs = reinterpret_cast<const LikTabs *>(ctx->log_tab);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(grid + n_b_blocks)), dim3(LIK_BLOCK), t.lds, s, bt, n_items, (int)U, (int)K, th, tabs,
                       t.rec_b, t.rec_bt, lM, (int)grid, b, C, (int)H, S_B, lp_B_g_F, slots);
    FCD_LAUNCH_CHECK();
    return sess_nan_fold(slots, n_missing2, s);
}

// the shared tables: K_lik_shared's grid (a lane group per edge and pass, then the S_B blocks) with the terms of `t`
int lik_shared_sessions_launch(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U, int64_t K,
                               const LikTheta &th, const SessTerms &t, double *S_B, double *L, int flags, int64_t *nan_counts,
                               hipStream_t s) {
    const int group = U <= 16 ? 16 : (U <= 32 ? 32 : 64);
    const auto kernel = (flags & FCD_DATA_NAN_MISSING) ? lik_shared_sessions_fn<true>(t.terms, group)
                                                       : lik_shared_sessions_fn<false>(t.terms, group);
    const int64_t epb = LIK_BLOCK / group;
    int64_t n_l = (C + epb - 1) / epb;               // one pass per block up to 16 blocks per CU, grid-stride beyond
    n_l = (n_l + t.per_block - 1) / t.per_block;
    const int64_t cap = (int64_t)ctx->num_cu * 16;
    if (n_l > cap) n_l = cap;
    const int64_t n_b_blocks = (C + 15) / 16;
    unsigned long long *slots = nan_counts ? reinterpret_cast<unsigned long long *>(ctx->nan_slots) : nullptr;
    const LikTabs *tabs = reinterpret_cast<const LikTabs *>(ctx->log_tab);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(n_l + n_b_blocks)), dim3(LIK_BLOCK), t.lds, s, bt, C, (int)U, (int)K, th, tabs,
                       t.rec_b, t.rec_bt, L, (int)n_l, b, (int)H, S_B, slots);
    FCD_LAUNCH_CHECK();
    return sess_nan_fold(slots, nan_counts, s);
}

template <bool MISSING>
auto lik_grouped_fn(int terms) {
    return terms == TERMS_SIGMA    ? lik_grouped_kernel<MISSING, TERMS_SIGMA>
           : terms == TERMS_GLOBAL ? lik_grouped_kernel<MISSING, TERMS_GLOBAL>
                                   : lik_grouped_kernel<MISSING, TERMS_LDS>;
}

// the grouped tables: a lane group per (edge, group) pair and pass, then the S_B blocks, with the terms of `t`.  The lane
// width is the kernel's to choose (it reads the largest group off `offsets`), so the grid is sized for the widest, 4 pairs
// per block: under the cap of 16 blocks per CU a narrower width leaves the last blocks without a pair, nothing more.
int lik_grouped_launch(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U, int64_t K,
                       const LikTheta &th, const SessTerms &t, const int32_t *order, const int64_t *offsets, int64_t G, double *S_B,
                       double *L, int flags, int64_t *nan_counts, hipStream_t s) {
    const auto kernel = (flags & FCD_DATA_NAN_MISSING) ? lik_grouped_fn<true>(t.terms) : lik_grouped_fn<false>(t.terms);
    const int64_t ppb = LIK_BLOCK / 64;
    int64_t n_l = (C * G + ppb - 1) / ppb;
    n_l = (n_l + t.per_block - 1) / t.per_block;
    const int64_t cap = (int64_t)ctx->num_cu * 16;
    if (n_l > cap) n_l = cap;
    const int64_t n_b_blocks = (C + 15) / 16;
    unsigned long long *slots = nan_counts ? reinterpret_cast<unsigned long long *>(ctx->nan_slots) : nullptr;
    const LikTabs *tabs = reinterpret_cast<const LikTabs *>(ctx->log_tab);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(n_l + n_b_blocks)), dim3(LIK_BLOCK), t.lds, s, bt, C, (int)U, (int)K, th, tabs,
                       t.rec_b, t.rec_bt, order, offsets, (int)G, L, (int)n_l, b, (int)H, S_B, slots);
    FCD_LAUNCH_CHECK();
    return sess_nan_fold(slots, nan_counts, s);
}

// both connection posteriors; who = the entry point's name, `records`: the terms come from var_bt's records (NULL: v = 0)
int conn_posterior_sessions(fcd_ctx *ctx, const char *who, bool records, const double *bt, int64_t Nreg, int64_t U, int64_t K,
                            const double *theta, const double *var_bt, const uint32_t *counts, const double *lq_F,
                            const double *lq_R, int flags, double *p_T, double *p_F_tilde, double *p_changed, hipStream_t s) {
    if (!ctx || !bt || !theta || !p_T || !p_F_tilde || !p_changed) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    if (flags & ~FCD_DATA_NAN_MISSING) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "unknown flags 0x%x", flags);
    if ((counts != nullptr) == (lq_F != nullptr || lq_R != nullptr) || (!counts && (!lq_F || !lq_R)))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "pass counts, or lq_F and lq_R");
    if (Nreg < 2 || U < 1 || U > INT32_MAX || Nreg > 46340) return fcd_fail_who(ctx, FCD_ERR_SHAPE, who, "Nreg=%lld U=%lld", Nreg, U);
    if (K < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "K=%lld sessions, must be >= 1", K);
    const int64_t C = fcd_tri(Nreg);
    if (K > INT32_MAX || C * U > INT64_MAX / 8 / K || (records && U * K > ((int64_t)1 << 31)))
        return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "K=%lld too large", K);
    SessPostTheta th;
    const double eta = theta[1], epsilon = theta[2];
    for (int k = 0; k < 3; ++k) {
        th.mu[k] = theta[6 + k];
        th.sigma[k] = theta[9 + k];
        th.lsigma[k] = log(th.sigma[k]);
        if (!(th.sigma[k] > 0.0)) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "sigma must be > 0");
    }
    th.eps = epsilon;
    th.e[0] = 1 - epsilon;                        // _eval_M_eps, fit.py:433-444
    th.e[1] = epsilon;
    double e2 = eta * epsilon;
    e2 += (1 - eta) * (1 - epsilon);
    th.e[2] = e2;
    th.pT[0] = 0.0;
    th.pT[1] = 1.0;
    th.pT[2] = eta;
    const NoiseRec *rec_b = nullptr, *rec_bt = nullptr;
    if (records) {
        LikTheta lt;
        lik_theta_make(theta, lt);
        int rc = noise_records(ctx, nullptr, var_bt, 1, U, K, lt, s, &rec_b, &rec_bt);
        if (rc) return rc;
    }
    const int64_t items = C * U;
    int64_t blocks = (items + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cu * 64;
    if (blocks > cap) blocks = cap;
    const bool miss = (flags & FCD_DATA_NAN_MISSING) != 0;
    const auto kernel = records ? (miss ? posterior_sessions_kernel<true, TERMS_GLOBAL> : posterior_sessions_kernel<false, TERMS_GLOBAL>)
                                : (miss ? posterior_sessions_kernel<true, TERMS_SIGMA> : posterior_sessions_kernel<false, TERMS_SIGMA>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, s, bt, C, (int)U, (int)K, th, rec_bt, counts, lq_F, lq_R, p_T,
                       p_F_tilde, p_changed);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

}  // namespace

extern "C" int fcd_lik_tables_sessions(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U, int64_t K,
                                       const double *theta, double *S_B, double *lM, double *lp_B_g_F, int flags,
                                       int64_t *n_missing2, fcd_stream stream) {
    if (!ctx || !b || !bt || !theta || !S_B || !lM) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_tables_sessions: null pointer");
    FCD_ALIGN16(ctx, "fcd_lik_tables_sessions", "lM", lM);          // lik_sessions_kernel stores it as double2
    int rc = sess_check(ctx, "sessions tables", false, C, H, U, K, flags, n_missing2 != nullptr);
    if (rc) return rc;
    LikTheta th;
    lik_theta_make(theta, th);
    return lik_sessions_launch(ctx, b, bt, C, H, U, K, th, SessTerms(), S_B, lM, lp_B_g_F, flags, n_missing2, (hipStream_t)stream);
}

extern "C" int fcd_lik_shared_tables_sessions(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                              int64_t K, const double *theta, double *S_B, double *L, int flags,
                                              int64_t *nan_counts, fcd_stream stream) {
    if (!ctx || !b || !bt || !theta || !S_B || !L) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_shared_tables_sessions: null pointer");
    int rc = sess_check(ctx, "sessions tables", false, C, H, U, K, flags, nan_counts != nullptr);
    if (rc) return rc;
    LikTheta th;
    lik_theta_make(theta, th);
    return lik_shared_sessions_launch(ctx, b, bt, C, H, U, K, th, SessTerms(), S_B, L, flags, nan_counts, (hipStream_t)stream);
}

extern "C" int fcd_conn_posterior_sessions(fcd_ctx *ctx, const double *bt, int64_t Nreg, int64_t U, int64_t K, const double *theta,
                                           const uint32_t *counts, const double *lq_F, const double *lq_R, int flags, double *p_T,
                                           double *p_F_tilde, double *p_changed, fcd_stream stream) {
    return conn_posterior_sessions(ctx, "fcd_conn_posterior_sessions", false, bt, Nreg, U, K, theta, nullptr, counts, lq_F, lq_R,
                                   flags, p_T, p_F_tilde, p_changed, (hipStream_t)stream);
}

// (both variance pointers NULL still takes the record form, with v = 0)
extern "C" int fcd_lik_tables_noise(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U, int64_t K,
                                    const double *theta, const double *var_b, const double *var_bt, double *S_B, double *lM,
                                    double *lp_B_g_F, int flags, int64_t *n_missing2, fcd_stream stream) {
    if (!ctx || !b || !bt || !theta || !S_B || !lM) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_tables_noise: null pointer");
    FCD_ALIGN16(ctx, "fcd_lik_tables_noise", "lM", lM);
    int rc = sess_check(ctx, "noise tables", true, C, H, U, K, flags, n_missing2 != nullptr);
    if (rc) return rc;
    LikTheta th;
    lik_theta_make(theta, th);
    SessTerms t;
    rc = noise_terms(ctx, var_b, var_bt, H, U, K, th, (hipStream_t)stream, t);
    if (rc) return rc;
    return lik_sessions_launch(ctx, b, bt, C, H, U, K, th, t, S_B, lM, lp_B_g_F, flags, n_missing2, (hipStream_t)stream);
}

extern "C" int fcd_lik_shared_tables_noise(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                           int64_t K, const double *theta, const double *var_b, const double *var_bt,
                                           double *S_B, double *L, int flags, int64_t *nan_counts, fcd_stream stream) {
    if (!ctx || !b || !bt || !theta || !S_B || !L) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_shared_tables_noise: null pointer");
    int rc = sess_check(ctx, "noise tables", true, C, H, U, K, flags, nan_counts != nullptr);
    if (rc) return rc;
    LikTheta th;
    lik_theta_make(theta, th);
    SessTerms t;
    rc = noise_terms(ctx, var_b, var_bt, H, U, K, th, (hipStream_t)stream, t);
    if (rc) return rc;
    return lik_shared_sessions_launch(ctx, b, bt, C, H, U, K, th, t, S_B, L, flags, nan_counts, (hipStream_t)stream);
}

// order and offsets are device arrays: their contents (a permutation of the patients, spans that start at 0, end at U and
// never shrink to nothing) are the caller's to check on its host copy before the upload; nothing here waits for the device
extern "C" int fcd_lik_grouped_tables(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U, int64_t K,
                                      const double *theta, const double *var_b, const double *var_bt, const int32_t *order,
                                      const int64_t *offsets, int64_t G, double *S_B, double *L, int flags, int64_t *nan_counts,
                                      fcd_stream stream) {
    if (!ctx || !b || !bt || !theta || !order || !offsets || !S_B || !L)
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_lik_grouped_tables: null pointer");
    const bool records = var_b || var_bt;
    int rc = sess_check(ctx, "grouped tables", records, C, H, U, K, flags, nan_counts != nullptr);
    if (rc) return rc;
    if (G < 1 || G > U) return fcd_fail(ctx, FCD_ERR_ARG, "grouped tables: G=%lld groups, must be 1 .. U=%lld", G, U);
    LikTheta th;
    lik_theta_make(theta, th);
    SessTerms t;
    if (records) {
        rc = noise_terms(ctx, var_b, var_bt, H, U, K, th, (hipStream_t)stream, t);
        if (rc) return rc;
    }
    return lik_grouped_launch(ctx, b, bt, C, H, U, K, th, t, order, offsets, G, S_B, L, flags, nan_counts, (hipStream_t)stream);
}

extern "C" int fcd_conn_posterior_noise(fcd_ctx *ctx, const double *bt, int64_t Nreg, int64_t U, int64_t K, const double *theta,
                                        const double *var_bt, const uint32_t *counts, const double *lq_F, const double *lq_R,
                                        int flags, double *p_T, double *p_F_tilde, double *p_changed, fcd_stream stream) {
    return conn_posterior_sessions(ctx, "fcd_conn_posterior_noise", true, bt, Nreg, U, K, theta, var_bt, counts, lq_F, lq_R,
                                   flags, p_T, p_F_tilde, p_changed, (hipStream_t)stream);
}
