// Many-chain collapsed Gibbs sampler over (f, r) for the IAR model, built on the reference's per-edge
// tables.  The two conditionals are fcdiff/fit.py:170-173 (f) and :187-194 (r) at one-hot q.
//
// Mapping: lane = chain.  A wave owns one "chain word" (64 chains); everything that does not depend
// on the chain (edge id, patient, region pair, table tile) is wave-uniform and lives in SGPRs / LDS:
//   * r is stored as bit planes r_bits[w][n][u] (one uint64 = r_nu of the 64 chains of word w), so
//     the mixture index l(r_nu, r_mu) of all 64 chains comes from two scalar masks and becomes a
//     per-lane LDS byte offset with two v_cndmask;
//   * f is stored as f_state[w][c][64] bytes: a wave reads/writes 64 contiguous bytes per edge.
//
// Algorithmic bytes per sweep of G chains: 2*72*C*U (lM once per pass) + 24*C +
// G*(2*C + 3*Nreg*U) of state.  Arithmetic: 3 (f) + 4 (r) fp64 adds per (edge, patient, chain).
#include "fcd_common.h"
#include <chrono>

namespace {

// ---------------------------------------------------------------------------------------------
// init
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gibbs_init_f(uint8_t *__restrict__ f_state, int64_t C, int GW, uint32_t chain0,
                                                    uint64_t seed) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // (w, pair of edges)
    const int64_t n_pairs = (C + 1) / 2;
    if (item >= n_pairs * GW) return;
    const int w = (int)(item / n_pairs);
    const int64_t pr = item % n_pairs;
    const uint32_t chain = chain0 + (uint32_t)w * 64u + lane;
    const fcd_u4 x = fcd_philox((uint32_t)pr, chain, 0u, FCD_KIND_INIT_F, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int f0 = min((int)(fcd_u53(x.x, x.y) * 3.0), 2);
    const int f1 = min((int)(fcd_u53(x.z, x.w) * 3.0), 2);
    const int64_t c = pr * 2;
    f_state[((int64_t)w * C + c) * 64 + lane] = (uint8_t)f0;
    if (c + 1 < C) f_state[((int64_t)w * C + c + 1) * 64 + lane] = (uint8_t)f1;
}

__global__ __launch_bounds__(256) void gibbs_init_r(uint64_t *__restrict__ r_bits, int Nreg, int U, int GW,
                                                    uint32_t chain0, uint64_t seed, double pi) {
    const int lane = threadIdx.x & 63;
    const int64_t n_np = (Nreg + 1) / 2;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // (w, region pair, u)
    if (item >= n_np * U * GW) return;
    const int w = (int)(item / (n_np * U));
    const int64_t rest = item % (n_np * U);
    const int np = (int)(rest / U), u = (int)(rest % U);
    const uint32_t chain = chain0 + (uint32_t)w * 64u + lane;
    const fcd_u4 x = fcd_philox((uint32_t)(np * U + u), chain, 0u, FCD_KIND_INIT_R, (uint32_t)seed,
                                (uint32_t)(seed >> 32));
    const uint64_t b0 = __ballot(fcd_u53(x.x, x.y) < pi);
    const uint64_t b1 = __ballot(fcd_u53(x.z, x.w) < pi);
    if (lane == 0) {
        const int n = np * 2;
        r_bits[((int64_t)w * Nreg + n) * U + u] = b0;
        if (n + 1 < Nreg) r_bits[((int64_t)w * Nreg + n + 1) * U + u] = b1;
    }
}

// ---------------------------------------------------------------------------------------------
// f step.  grid.x = edge tiles of Ec edges, grid.y = groups of (blockDim/64) chain words.
// The tile lM[c0 : c0+Ec, :, :, :] (contiguous, Ec*U*72 bytes) is staged in LDS once and read by every
// wave of the block: with 16 waves (1024 chains) per block the table is read from HBM/L2 once per pass.
// COND = true writes the three unnormalised log-weights instead of drawing (parity hook).
// ---------------------------------------------------------------------------------------------
constexpr int F_UNROLL = 8;
template <bool COND>
__global__ __launch_bounds__(1024) void gibbs_f_kernel(const double *__restrict__ S_B, const double *__restrict__ lM,
                                                       const double *__restrict__ hyper, uint8_t *__restrict__ f_state,
                                                       const uint64_t *__restrict__ r_bits, int Nreg, int U, int64_t C,
                                                       int GW, int64_t G, int Ec, uint32_t chain0, uint64_t seed,
                                                       uint32_t sweep, double *__restrict__ cond_f) {
    extern __shared__ double tile[];
    const int64_t c0 = (int64_t)blockIdx.x * Ec;
    const int ne = (int)((C - c0 < Ec) ? (C - c0) : Ec);
    {
        const int64_t n_dbl = (int64_t)ne * U * 9;
        const double *src = lM + c0 * U * 9;
        for (int64_t i = threadIdx.x; i < n_dbl; i += blockDim.x) tile[i] = src[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    if (w >= GW) return;
    const uint32_t chain = chain0 + (uint32_t)w * 64u + lane;
    const double lng0 = hyper[FCD_H_LNGAMMA + 0], lng1 = hyper[FCD_H_LNGAMMA + 1], lng2 = hyper[FCD_H_LNGAMMA + 2];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint64_t *__restrict__ rw = r_bits + (int64_t)w * Nreg * U;
    fcd_u4 rnd = {0, 0, 0, 0};
    int64_t rnd_idx = -1;

    for (int e = 0; e < ne; ++e) {
        const int64_t c = c0 + e;
        int n, m;
        fcd_edge_to_pair(c, n, m);
        const uint64_t *__restrict__ rn = rw + (int64_t)n * U;
        const uint64_t *__restrict__ rm = rw + (int64_t)m * U;
        const char *tb = reinterpret_cast<const char *>(tile + (int64_t)e * U * 9);
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        // l = 1 (both anomalous) -> +8 B, l = 2 (discordant) -> +16 B, l = 0 -> +0 inside lM[c,u,k,:].
        // Chunks of F_UNROLL patients with a fixed trip count: the masks of a chunk arrive in one wide
        // scalar load per region and the LDS reads of a chunk are all in flight together.
        int u = 0;
        for (; u + F_UNROLL <= U; u += F_UNROLL) {
#pragma unroll
            for (int j = 0; j < F_UNROLL; ++j) {
                const uint64_t mn = rn[u + j], mm = rm[u + j];
                const uint32_t off = fcd_sel_mask(fcd_sel_mask(0u, 16u, mn ^ mm), 8u, mn & mm);
                const double *p = reinterpret_cast<const double *>(tb + (u + j) * 72 + off);
                a0 += p[0];
                a1 += p[3];
                a2 += p[6];
            }
        }
        for (; u < U; ++u) {
            const uint64_t mn = rn[u], mm = rm[u];
            const uint32_t off = fcd_sel_mask(fcd_sel_mask(0u, 16u, mn ^ mm), 8u, mn & mm);
            const double *p = reinterpret_cast<const double *>(tb + u * 72 + off);
            a0 += p[0];
            a1 += p[3];
            a2 += p[6];
        }
        a0 = lng0 + (S_B[c * 3 + 0] + a0);   // fit.py:165, 171-173
        a1 = lng1 + (S_B[c * 3 + 1] + a1);
        a2 = lng2 + (S_B[c * 3 + 2] + a2);
        if (COND) {
            if ((int64_t)w * 64 + lane < G) {
                double *o = cond_f + (((int64_t)w * 64 + lane) * C + c) * 3;
                o[0] = a0; o[1] = a1; o[2] = a2;
            }
        } else {
            if ((c >> 2) != rnd_idx) {
                rnd_idx = c >> 2;
                rnd = fcd_philox((uint32_t)rnd_idx, chain, sweep, FCD_KIND_F, k0, k1);
            }
            const double x = fcd_u32(fcd_word(rnd, (int)(c & 3)));
            f_state[((int64_t)w * C + c) * 64 + lane] = (uint8_t)fcd_draw_f(a0, a1, a2, x);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// f step, difference form.  Only the two log-odds b_k = a_k - a_0, k = 1, 2 enter the draw, and
//   b_k = ln(gamma_k/gamma_0) + (S_B[c,k] - S_B[c,0]) + sum_u lMf[c,u,l_u,k-1],
//   lMf[c,u,l,k-1] = lM[c,u,k,l] - lM[c,u,0,l]            (edge-major difference table, 48 B per (c,u))
// so a term is one 16-byte LDS read and two fp64 adds.  Same tiling as gibbs_f_kernel.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void edge_tables_kernel(const double *__restrict__ lM, int64_t n_items,
                                                          double *__restrict__ lMf) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * blockDim.x) {
        const double *p = lM + i * 9;
        double *o = lMf + i * 6;
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            o[l * 2 + 0] = p[3 + l] - p[l];
            o[l * 2 + 1] = p[6 + l] - p[l];
        }
    }
}

// (the lanes whose log-odds are not finite, and their draw from the absolute log-weights: defined with the pair forms below)
__device__ __forceinline__ bool fcd_f_open(double b1, double b2);
__device__ int fcd_f_abs_edge_masks(const double *__restrict__ row9, const double *__restrict__ sb, const double *__restrict__ hyper,
                                    const uint64_t *__restrict__ rn, const uint64_t *__restrict__ rm, int U, int lane, double x);

__global__ __launch_bounds__(1024) void gibbs_f_diff_kernel(const double *__restrict__ S_B, const double *__restrict__ lMf,
                                                            const double *__restrict__ hyper, uint8_t *__restrict__ f_state,
                                                            const uint64_t *__restrict__ r_bits, int Nreg, int U, int64_t C,
                                                            int GW, int Ec, uint32_t chain0, uint64_t seed, uint32_t sweep,
                                                            float margin, const double *__restrict__ lM) {
    extern __shared__ __attribute__((aligned(16))) double tile[];   // [Ec][U][3][2]
    const int64_t c0 = (int64_t)blockIdx.x * Ec;
    const int ne = (int)((C - c0 < Ec) ? (C - c0) : Ec);
    {
        const int n_d2 = ne * U * 3;
        const double2 *src = reinterpret_cast<const double2 *>(lMf + c0 * U * 6);
        double2 *dst = reinterpret_cast<double2 *>(tile);
        for (int i = threadIdx.x; i < n_d2; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    if (w >= GW) return;
    const uint32_t chain = chain0 + (uint32_t)w * 64u + lane;
    const double lg1 = hyper[FCD_H_LNGAMMA + 1] - hyper[FCD_H_LNGAMMA + 0];
    const double lg2 = hyper[FCD_H_LNGAMMA + 2] - hyper[FCD_H_LNGAMMA + 0];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint64_t *__restrict__ rw = r_bits + (int64_t)w * Nreg * U;
    fcd_u4 rnd = {0, 0, 0, 0};
    int64_t rnd_idx = -1;
    if (FCD_ABL(0, 3)) return;           // ablation: staging only

    for (int e = 0; e < ne; ++e) {
        const int64_t c = c0 + e;
        int n, m;
        fcd_edge_to_pair(c, n, m);
        const uint64_t *__restrict__ rn = rw + (int64_t)n * U;
        const uint64_t *__restrict__ rm = rw + (int64_t)m * U;
        const char *tb = reinterpret_cast<const char *>(tile) + (int64_t)e * U * 48;
        double b1 = 0.0, b2 = 0.0;
        int u = 0;
        for (; u + F_UNROLL <= U; u += F_UNROLL) {
#pragma unroll
            for (int j = 0; j < F_UNROLL; ++j) {
                const uint64_t mn = rn[u + j], mm = rm[u + j];
                // l = 1 (both anomalous) -> +16 B, l = 2 (discordant) -> +32 B, l = 0 -> +0 inside lMf[c,u,:,:]
                const uint32_t off = fcd_sel_mask(fcd_sel_mask(0u, 32u, mn ^ mm), 16u, mn & mm);
                const double2 v = *reinterpret_cast<const double2 *>(tb + (u + j) * 48 + off);
                b1 += v.x;
                b2 += v.y;
            }
        }
        for (; u < U; ++u) {
            const uint64_t mn = rn[u], mm = rm[u];
            const uint32_t off = fcd_sel_mask(fcd_sel_mask(0u, 32u, mn ^ mm), 16u, mn & mm);
            const double2 v = *reinterpret_cast<const double2 *>(tb + u * 48 + off);
            b1 += v.x;
            b2 += v.y;
        }
        b1 = lg1 + ((S_B[c * 3 + 1] - S_B[c * 3 + 0]) + b1);
        b2 = lg2 + ((S_B[c * 3 + 2] - S_B[c * 3 + 0]) + b2);
        if (FCD_ABL(0, 2)) {             // ablation: no RNG / exp
            f_state[((int64_t)w * C + c) * 64 + lane] = (uint8_t)(b1 > b2 ? 1 : 2);
            continue;
        }
        if ((c >> 2) != rnd_idx) {
            rnd_idx = c >> 2;
            rnd = fcd_philox((uint32_t)rnd_idx, chain, sweep, FCD_KIND_F, k0, k1);
        }
        const double x = fcd_u32(fcd_word(rnd, (int)(c & 3)));
        bool amb;
        int k = fcd_draw_f_fast(b1, b2, x, 2e-5f, margin, &amb);
        if (__ballot(amb) != 0ull) {                                     // too close to a boundary somewhere in the wave
            k = fcd_draw_f(0.0, b1, b2, x);
            const bool open = fcd_f_open(b1, b2);                       // (type 0 impossible: the absolute log-weights decide)
            if (__ballot(open) != 0ull) {
                const int ka = fcd_f_abs_edge_masks(lM + c * U * 9, S_B + c * 3, hyper, rn, rm, U, lane, x);
                if (open) k = ka;
            }
        }
        f_state[((int64_t)w * C + c) * 64 + lane] = (uint8_t)k;
    }
}

// ---------------------------------------------------------------------------------------------
// f step, pair form (U <= 64).  The kernel is bound by wave-wide LDS reads (one per gathered value whatever
// the number of distinct addresses: profiles/r01_ubench_lds_fp64.txt), so the tile holds records for PAIRS of
// patients (u, u+1): for each of the 16 values of (x_u, x_u+1, a_u, a_u+1), x = r_n xor r_m, a = r_n and r_m,
//   rec[slot] = lMf[c][u][l(x_u, a_u)][:] + lMf[c][u+1][l(x_u+1, a_u+1)][:]        (2 doubles, 256 B per pair)
// built in LDS while staging.  One ds_read_b128 + two fp64 adds then cover two patients.  r comes as per-lane
// words over patients (r_U, made by pack_ru_kernel): no scalar loads inside the loop.  A word holds 16 patients
// SPREAD over 4-bit fields, the pair (u, u+1) in the low two bits of field u/2: (r_n ^ r_m) | (r_n & r_m) << 2 is
// then the slot number of every pair at once, and a term costs two integer instructions for its address.
// ---------------------------------------------------------------------------------------------
// One slot-source word of (w, n): 16 patients in 4-bit fields (the pair (u, u+1) in the low two bits of field u/2).
// Where slot word jw of (w, n) = wn lives for lane: the words of a region are kept FOUR side by side per lane (round 4), so
// that one 16-byte load fetches what four 4-byte loads did -- a vector-memory instruction occupies the CU's address unit
// for the same ~16 cycles whatever its width (profiles/r04_ubench_vmem_rate.txt), and the pair kernel issued eight per edge.
// (NW <= 4, the U <= 64 kernel: side by side.  The any-U kernel consumes one word per loop turn and keeps [word][lane]: with
// the 16-byte words held across four turns it measured 1.83 against 1.72 ms at cfg5.)
__host__ __device__ static inline int64_t ru_index(int64_t wn, int NW, int jw, int lane) {
    return NW <= 4 ? (wn * 64 + lane) * 4 + jw : (wn * NW + jw) * 64 + lane;
}
// (the whole wave, (wn, jw) wave-uniform: lane l loads the word of patient 16 jw + l % 16 -- one memory instruction instead of 16)
__device__ __forceinline__ uint32_t pack_ru_word(const uint64_t *__restrict__ r_bits, int64_t wn, int U, int jw, int lane) {
    const int ul = jw * 16 + (lane & 15);
    const uint64_t mine = r_bits[wn * U + (ul < U ? ul : U - 1)];                                  // clamped: no branch around the load
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int u = jw * 16 + j;
        v |= (u < U ? (uint32_t)((fcd_lane_word(mine, j) >> lane) & 1ull) : 0u) << (4 * (j >> 1) + (j & 1));
    }
    return v;
}
__global__ __launch_bounds__(256) void pack_ru_kernel(const uint64_t *__restrict__ r_bits, int Nreg, int U, int NW, int GW,
                                                      uint32_t *__restrict__ r_U) {
    const int lane = threadIdx.x & 63;
    const int item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));      // (w, n, word): scalar
    if (item >= GW * Nreg * NW) return;
    const int jw = item % NW, wn = item / NW;                   // wn = w*Nreg + n
    r_U[ru_index(wn, NW, jw, lane)] = pack_ru_word(r_bits, wn, U, jw, lane);
}

typedef float fcd_f2v __attribute__((ext_vector_type(2)));           // one ds_read_b64, one v_pk_add_f32
typedef __attribute__((address_space(3))) const fcd_f2v lds_cf2v;
typedef float fcd_f4v __attribute__((ext_vector_type(4)));

// 16-byte piece s2 of the record of a pair of patients (slots 2 s2, 2 s2 + 1 of its 16: bit 0 / 1 = x of patient u / u + 1,
// bit 2 / 3 = a): the sums of the two patients' rows A, B (the three mixture cases: 0 typical, 1 both, 2 discordant) in
// fp64, rounded once to fp32; zeros for the seven impossible slots (x and a both set for a patient).
__device__ __forceinline__ fcd_f4v fp_pair_piece(const double2 (&A)[3], const double2 (&B)[3], int s2) {
    fcd_f4v o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int slot = 2 * s2 + h;
        const int x0 = slot & 1, x1 = (slot >> 1) & 1, a0 = (slot >> 2) & 1, a1 = slot >> 3;
        const bool valid = !((x0 & a0) | (x1 & a1));
        const int l0 = a0 ? 1 : (x0 ? 2 : 0), l1 = a1 ? 1 : (x1 ? 2 : 0);
        const float vx = valid ? (float)(A[l0].x + B[l1].x) : 0.f, vy = valid ? (float)(A[l0].y + B[l1].y) : 0.f;
        if (h == 0) { o.x = vx; o.y = vy; } else { o.z = vx; o.w = vy; }
    }
    return o;
}
// B_e >= sum over the pairs of max |record entry|: the sum over the patients of the largest |value| of the row (the whole
// wave; lane = patient, su = its row, live = lane < U <= 64) -- what bounds the error of the fp32 sums of the term loop
__device__ __forceinline__ float fp_edge_bound(const double2 *su, bool live) {
    float a = 0.f;
    if (live) {
#pragma unroll
        for (int l = 0; l < 3; ++l) a = fmaxf(a, fmaxf((float)fabs(su[l].x), (float)fabs(su[l].y)));
        a *= 1.0000002f;                              // (the conversions of the records round to nearest)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    return a;
}

// The exact path of the pair forms: the two log-odds sums of edge c for this lane's chain in fp64, straight from the
// table (48 contiguous bytes per patient: L2), in the order of the fp64 pair records of rounds 2-3 (record = row u + row
// u+1, records summed in pair order).  zs: the slot word of a group of 8 pairs, np pairs of it used.
__device__ __forceinline__ void fcd_f_exact_group(const double *__restrict__ row, int U, int u0, int np, uint32_t zs,
                                                  bool &first, double &b1, double &b2) {
#pragma unroll 1
    for (int p = 0; p < np; ++p) {
        const uint32_t f = (zs >> (4 * p)) & 15u;
        const int l0 = (f & 4u) ? 1 : ((f & 1u) ? 2 : 0), l1 = (f & 8u) ? 1 : ((f & 2u) ? 2 : 0);   // 0 typical, 1 both, 2 discordant
        const int u = u0 + 2 * p;
        const double2 va = *reinterpret_cast<const double2 *>(row + ((int64_t)u * 3 + l0) * 2);
        double r1 = va.x, r2 = va.y;
        if (u + 1 < U) {
            const double2 vb = *reinterpret_cast<const double2 *>(row + ((int64_t)(u + 1) * 3 + l1) * 2);
            r1 += vb.x;
            r2 += vb.y;
        }
        if (first) {
            b1 = r1;
            b2 = r2;
            first = false;
        } else {
            b1 += r1;
            b2 += r2;
        }
    }
}

// Log-odds against type 0 say nothing where type 0 itself is impossible: a0 = -inf (gamma_0 = 0, or an entry lM[c][u][0][l] =
// -inf of a density that underflowed) makes b1, b2 +inf or NaN, and fcd_draw_f(0, b1, b2, x) then answers 2 whatever the
// weights of types 1 and 2.  The law is fcd_draw_f of the ABSOLUTE log-weights, as gibbs_f_kernel and the oracle make them:
// a_k = ln gamma_k + (S_B[c][k] + sum_u lM[c][u][k][l_u]), the sum in the order of the patients from 0.0.  The exact repeats of
// the log-odds forms end here for the lanes whose b1 or b2 is not finite (fcd_f_open); an edge without such a lane -- every
// edge of finite tables and positive gamma -- never comes here.  Three gathers of the row lM[c] (72 bytes per patient: L2), by
// what the form holds of the r state: slot words of 8 pairs of patients, or the bit planes.
__device__ __forceinline__ bool fcd_f_open(double b1, double b2) { return !(isfinite(b1) && isfinite(b2)); }
__device__ __forceinline__ void fcd_f_abs_group(const double *__restrict__ row9, int U, int u0, int np, uint32_t zs, double (&a)[3]) {
#pragma unroll 1
    for (int p = 0; p < np; ++p) {
        const uint32_t f = (zs >> (4 * p)) & 15u;
        const int l0 = (f & 4u) ? 1 : ((f & 1u) ? 2 : 0), l1 = (f & 8u) ? 1 : ((f & 2u) ? 2 : 0);   // 0 typical, 1 both, 2 discordant
        const int u = u0 + 2 * p;
        const double *q = row9 + (int64_t)u * 9 + l0;
        a[0] += q[0]; a[1] += q[3]; a[2] += q[6];
        if (u + 1 < U) {
            const double *q1 = row9 + (int64_t)(u + 1) * 9 + l1;
            a[0] += q1[0]; a[1] += q1[3]; a[2] += q1[6];
        }
    }
}
__device__ __forceinline__ int fcd_f_abs_draw(const double *__restrict__ sb, const double *__restrict__ hyper, const double (&a)[3], double x) {
    return fcd_draw_f(hyper[FCD_H_LNGAMMA + 0] + (sb[0] + a[0]), hyper[FCD_H_LNGAMMA + 1] + (sb[1] + a[1]),
                      hyper[FCD_H_LNGAMMA + 2] + (sb[2] + a[2]), x);
}
// (the scalar-mask form: rn, rm = the bit planes of the edge's two regions, one word per patient, bit = lane)
__device__ __attribute__((noinline)) int fcd_f_abs_edge_masks(const double *__restrict__ row9, const double *__restrict__ sb,
                                                              const double *__restrict__ hyper, const uint64_t *__restrict__ rn,
                                                              const uint64_t *__restrict__ rm, int U, int lane, double x) {
    double a[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int u = 0; u < U; ++u) {
        const int bn = (int)((rn[u] >> lane) & 1ull), bm = (int)((rm[u] >> lane) & 1ull);
        const double *q = row9 + (int64_t)u * 9 + ((bn & bm) ? 1 : ((bn ^ bm) ? 2 : 0));
        a[0] += q[0]; a[1] += q[3]; a[2] += q[6];
    }
    return fcd_f_abs_draw(sb, hyper, a, x);
}

// The exact path of the U <= 64 kernel as ONE out-of-line function: inlined into the eight unrolled edge bodies it was most of
// the kernel's text (fp64 exponentials, the gather loop), and the hot path had to be fetched around it.
// Returns the draw, + FCD_F_OPEN in the lanes of fcd_f_open.  The kernel notes those lanes per edge in the spare half of its
// word of draws and, AFTER its edge loop, asks fcd_f_abs_edge for each noted edge: the call inside the unrolled edge bodies
// keeps its arguments, and what the second call needs (the tables, the edge, the lane's chain) lives through the whole kernel
// anyway -- the registers of the edge loop stay what they were.
constexpr int FCD_F_OPEN = 4;
__device__ __attribute__((noinline)) int fcd_f_exact_edge(const double *__restrict__ row, double c1, double c2, uint32_t z0, uint32_t z1,
                                                          uint32_t z2, uint32_t z3, int U, uint32_t xw) {
    const int NPAIR = (U + 1) >> 1, NG = (NPAIR + 7) >> 3;
    bool first = true;
    double b1 = 0.0, b2 = 0.0;
#pragma unroll 1
    for (int g = 0; g < NG; ++g) {
        const uint32_t zs = g == 0 ? z0 : g == 1 ? z1 : g == 2 ? z2 : z3;
        fcd_f_exact_group(row, U, 16 * g, min(8, NPAIR - 8 * g), zs, first, b1, b2);
    }
    b1 = c1 + b1;
    b2 = c2 + b2;
    return fcd_draw_f(0.0, b1, b2, fcd_u32(xw)) | (fcd_f_open(b1, b2) ? FCD_F_OPEN : 0);
}
// Edge c = (n, m) of the U <= 64 kernel from the absolute log-weights, for this lane's chain: the slot words of the two regions
// (ru: the chain word's, four side by side per region and lane -- ru_index) and the draw's Philox word are made again.
__device__ __attribute__((noinline)) int fcd_f_abs_edge(const double *__restrict__ lM, const double *__restrict__ S_B,
                                                        const double *__restrict__ hyper, const uint4 *__restrict__ ru, int64_t c, int n,
                                                        int m, int U, uint32_t chain, uint32_t sweep, uint64_t seed) {
    const int NPAIR = (U + 1) >> 1, NG = (NPAIR + 7) >> 3;
    const uint32_t lane = threadIdx.x & 63u;
    const uint4 vn = ru[(uint32_t)(n * 64) + lane], vm = ru[(uint32_t)(m * 64) + lane];
    double a[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int g = 0; g < NG; ++g) {
        const uint32_t rn = g == 0 ? vn.x : g == 1 ? vn.y : g == 2 ? vn.z : vn.w, rm = g == 0 ? vm.x : g == 1 ? vm.y : g == 2 ? vm.z : vm.w;
        fcd_f_abs_group(lM + c * U * 9, U, 16 * g, min(8, NPAIR - 8 * g), (rn ^ rm) | ((rn & rm) << 2), a);
    }
    const fcd_u4 rnd = fcd_philox((uint32_t)(c >> 2), chain, sweep, FCD_KIND_F, (uint32_t)seed, (uint32_t)(seed >> 32));
    return fcd_f_abs_draw(S_B + c * 3, hyper, a, fcd_u32(fcd_word(rnd, (int)(c & 3))));
}

// Pair-aligned tiles (PT): tile t is rows (n0, n0 + 1) = (2i, 2i + 1) of the triangle x columns [mb, mb + FT_W) inside
// one block of 16 regions, edge e of the tile = (n0 + e / FT_W, mb + e % FT_W).  Row pair i has columns [0, n0 + 2) in
// floor(i/2) + 1 tiles, so the tiles before row pair i number j(j+1) (i = 2j) or (j+1)^2 (i = 2j+1).  A tile then holds both
// regions of every pair (m, m+1) of its rows and of every pair (n0, n0+1) of its columns: it writes the r pass's f words
// (f_S, pack_f_item) in their final form -- the row half into f_S[w][n][b(m)], the column half into f_S[w][m][b(n0)] --
// instead of the square copy the packing launch would read back.
// (FT_W, fpt_tiles: fcd_common.h)
struct fpt_tile {
    int n0, mb;
    int cnt0, cnt1;          // edges of row n0 / n0 + 1 in the tile (m < n, row inside the triangle)
    int64_t cr0, cr1;        // edge id of the first column of each row
};
__device__ __forceinline__ fpt_tile fpt_locate(int t, int Nreg) {
    int j = (int)((sqrtf(4.f * (float)t + 1.f) - 1.f) * 0.5f);
    while ((int64_t)(j + 1) * (j + 2) <= t) ++j;
    while ((int64_t)j * (j + 1) > t) --j;
    const int t0 = j * (j + 1);
    const int i = (t - t0 < j + 1) ? 2 * j : 2 * j + 1;
    fpt_tile T;
    T.n0 = 2 * i;
    T.mb = FT_W * (t - (int)fpt_tiles(i));
    T.cnt0 = min(FT_W, T.n0 - T.mb);
    T.cnt1 = T.n0 + 1 < Nreg ? min(FT_W, T.n0 + 1 - T.mb) : 0;
    T.cr0 = ((int64_t)T.n0 * (T.n0 - 1) >> 1) + T.mb;
    T.cr1 = T.cr0 + T.n0;
    return T;
}

// The r pass's f words of a pair-aligned tile from its draws kt (2 bits per edge), for this lane's chain of chain word w.
// (ROWS = false: without the row halves -- gibbs_f_run_kernel writes those of a full run itself, eight bytes at a time)
template <bool ROWS = true>
__device__ __forceinline__ void fpt_write_f_words(const fpt_tile &T, uint32_t kt, int w, int lane, uint2 *__restrict__ f_S, int Nreg, int NBLK) {
    // the r pass's f words (pack_f_item's bytes, (3 f(n, m) + f(n, m+1)) << 2; 0 for m == n and m >= Nreg).  K(r, j):
    // f of (n0 + r, mb + j) -- drawn here, 0 on the diagonal and for a row beyond Nreg, and (n0, n0 + 1) is the edge
    // (n0 + 1, n0) of row 1.  Every byte of f_S is written once per pass: the pairs of a row below its own row pair by the
    // row halves, the diagonal pair (n0, n0 + 1) by the row halves of the tile that holds it, the pairs above by the
    // column halves, the pairs beyond Nreg by the zeros of the diagonal tiles.
    auto K = [&](int r, int j) -> uint32_t {
        if (r == 0 && T.mb + j == T.n0 + 1) return (kt >> (2 * (FT_W + j - 1))) & 3u;
        return (kt >> (2 * (r * FT_W + j))) & 3u;
    };
    const int ncol = min(FT_W, T.n0 + 2 - T.mb);           // columns of the tile (FT_W, or 2 on the diagonal)
    const int b = T.mb / R_NB, p0 = (T.mb % R_NB) / 2;
    uint8_t *fs = reinterpret_cast<uint8_t *>(f_S + (int64_t)w * Nreg * NBLK * 64 + lane);     // + ((n * NBLK + b) * 64) * 8
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (!ROWS || T.n0 + r >= Nreg) break;
        uint8_t *row = fs + (int64_t)((T.n0 + r) * NBLK + b) * 512 + p0;
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < FT_W / 2; ++q) v |= ((3u * K(r, 2 * q) + K(r, 2 * q + 1)) << 2) << (8 * q);
        if (ncol == FT_W) *reinterpret_cast<uint16_t *>(row) = (uint16_t)v;     // (FT_W = 4: two bytes, 2-aligned)
        else *row = (uint8_t)v;
    }
    {
        const int bn = T.n0 / R_NB, pn = (T.n0 % R_NB) / 2;
#pragma unroll
        for (int j = 0; j < FT_W; ++j)
            if (T.mb + j < T.n0) fs[(int64_t)((T.mb + j) * NBLK + bn) * 512 + pn] = (uint8_t)((3u * K(0, j) + K(1, j)) << 2);
    }
    if (ncol < FT_W || T.mb + FT_W == T.n0 + 2) {
        // the diagonal tile of the row pair: the pairs of its rows beyond Nreg (last block)
        const int pe = (Nreg + 1) / 2 - (R_NB / 2) * (NBLK - 1);
        for (int r = 0; r < 2; ++r) {
            if (T.n0 + r >= Nreg) break;
            uint8_t *row = fs + (int64_t)((T.n0 + r) * NBLK + NBLK - 1) * 512;
            for (int p = pe; p < R_NB / 2; ++p) row[p] = 0;
        }
    }
}

// PRE (pair-aligned tiles only): the records and the edges' bounds come from the table gibbs_f_records_kernel made for this call
// (frec: per tile NPAIR x FP_EC records of F_REC_PIECES 16-byte pieces, then one fcd_f_edge_rec per edge id) -- one copy
// into LDS and ONE barrier instead of staging, barrier, build, barrier; no fp64 rows in LDS.
// SURE (with PRE; the host takes it where the table has such tiles, margin <= 1 and knob f_sure is not 1): a tile whose
// present edges are all decided by the table's bounds and this sweep's hyper (fcd_f_edge_mode) draws no sums.  The parent
// path would have taken fcd_draw_f_sure on every such edge, in every lane whose uniform lies in its range, so the waves draw
// the tile's Philox words as the edge loop does and test that range only; one vote of the workgroup (a word per wave behind
// the edge constants, one barrier) and, if no lane anywhere is out of range, k = the edge's mode: no slot words, no record
// copy, no term loops.  Otherwise the WHOLE tile runs the code below unchanged -- same draws, same repeats.  The rule's
// inputs and instructions are the same in all waves of a workgroup (w >= GW included), so all of them meet the barrier or none.
template <int NW16, bool PT, bool PRE = false, bool SURE = false>
__global__ __launch_bounds__(1024, 8) void gibbs_f_pair_kernel(const double *__restrict__ S_B, const double *__restrict__ lMf,
                                                            const double *__restrict__ hyper, uint8_t *__restrict__ f_state,
                                                            const uint32_t *__restrict__ r_U, int Nreg, int U, int64_t C,
                                                            int GW, uint32_t chain0, uint64_t seed, uint32_t sweep, float margin, uint8_t *__restrict__ fsq,
                                                            uint2 *__restrict__ f_S, int NBLK, fcd_dev_words *__restrict__ dbg,
                                                            const char *__restrict__ frec, const double *__restrict__ lM) {
    static_assert(PT || !PRE, "prebuilt records are laid out by pair-aligned tile");
    static_assert(PRE || !SURE, "the edges' bounds are part of the prebuilt records");
    // pair records [NPAIR][FP_EC][16] float2 | per-edge constants [FP_EC] float4 | (PRE) 16 vote words | (not PRE) singles [FP_EC][U][3][2] double
    extern __shared__ __attribute__((aligned(256))) double ptile[];
    const int NPAIR = (U + 1) >> 1;
    // the tile's edges: c0 + e, e < ne (consecutive ids); PT: edge e = (row e / FT_W, column e % FT_W), present where
    // e % FT_W < cnt of its row, id cr + e % FT_W
    const int64_t c0 = PT ? 0 : (int64_t)blockIdx.x * FP_EC;
    const fpt_tile T = PT ? fpt_locate((int)blockIdx.x, Nreg) : fpt_tile{0, 0, 0, 0, 0, 0};
    const int ne = PT ? FP_EC : (int)((C - c0 < FP_EC) ? (C - c0) : FP_EC);
    auto has = [&](int e) -> bool { return !PT ? e < ne : (e % FT_W) < (e < FT_W ? T.cnt0 : T.cnt1); };
    auto cid = [&](int e) -> int64_t { return !PT ? c0 + e : (e < FT_W ? T.cr0 : T.cr1) + (e % FT_W); };
    float4 *edge_k = reinterpret_cast<float4 *>(reinterpret_cast<char *>(ptile) + (size_t)FP_EC * NPAIR * 128);
    double2 *single = reinterpret_cast<double2 *>(reinterpret_cast<char *>(edge_k) + FP_EC * 16);
    const double lg1 = hyper[FCD_H_LNGAMMA + 1] - hyper[FCD_H_LNGAMMA + 0];
    const double lg2 = hyper[FCD_H_LNGAMMA + 2] - hyper[FCD_H_LNGAMMA + 0];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    [[maybe_unused]] const int trec = (int)blockIdx.x < 4096 ? (int)blockIdx.x : 4095;      // (diagnostic build: profiles/trace_f.py)
    FCD_TRACE(trec, 0);
    FCD_TRACE_VAL(trec, 7, (__builtin_amdgcn_s_getreg((31 << 11) | 20) << 16) | (__builtin_amdgcn_s_getreg((31 << 11) | 4) & 0xffff));
    if constexpr (SURE) {
        // lane e < FP_EC of every wave: edge e's rule
        const fcd_f_edge_rec *edge_c = reinterpret_cast<const fcd_f_edge_rec *>(frec + (size_t)gridDim.x * NPAIR * (FP_EC * F_REC_PIECES * 16));
        const int le = lane & (FP_EC - 1);
        const bool present = lane < FP_EC && has(le);
        int mode = -1;
        if (present) {
            const fcd_f_edge_rec k = edge_c[cid(le)];
            const double c1 = lg1 + k.d1, c2 = lg2 + k.d2;
            mode = fcd_f_edge_mode(c1, c2, k.b, fcd_f_edge_delta(c1, c2, NPAIR, k.a), FCD_F_SURE_T);
        }
        const uint32_t pm = (uint32_t)__ballot(present), dm = (uint32_t)__ballot(mode >= 0);
        if (pm != 0u && dm == pm) {           // (workgroup-uniform)
            const uint32_t m1 = (uint32_t)__ballot(mode == 1), m2 = (uint32_t)__ballot(mode == 2);
            bool out = false;               // this lane's uniform of some edge is outside fcd_draw_f_sure's range
            if (w < GW) {
                const uint32_t chain = chain0 + (uint32_t)w * 64u + lane;
                fcd_u4 rnd = {0, 0, 0, 0};
                int64_t rnd_blk = -1;
#pragma unroll
                for (int e = 0; e < FP_EC; ++e) {
                    if (!has(e)) continue;
                    const int64_t c = cid(e);
                    if ((c >> 2) != rnd_blk) {
                        rnd_blk = c >> 2;
                        rnd = fcd_philox((uint32_t)rnd_blk, chain, sweep, FCD_KIND_F, (uint32_t)seed, (uint32_t)(seed >> 32));
                    }
                    const float xf = (float)fcd_word(rnd, (int)(c & 3)) * 2.3283064e-10f;
                    out = out || !(xf > 1e-6f && xf < 0.999999f);
                }
            }
            uint32_t *vote = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(edge_k) + FP_EC * 16);
            const bool wave_out = __ballot(out) != 0ull;
            if (lane == 0) vote[threadIdx.x >> 6] = wave_out ? 1u : 0u;
            __syncthreads();
            const bool back = __ballot(lane < (int)(blockDim.x >> 6) && vote[lane < 16 ? lane : 0] != 0u) != 0ull;
            if (!back) {
                if (threadIdx.x == 0) atomicAdd(&dbg->f_sure_tiles, 1ull);
                if (w >= GW) return;
                uint32_t kt = 0;
#pragma unroll
                for (int e = 0; e < FP_EC; ++e) {
                    if (!has(e)) continue;
                    const uint32_t k = ((m1 >> e) & 1u) | (((m2 >> e) & 1u) << 1);
                    (f_state + ((int64_t)w * C + cid(e)) * 64)[(uint32_t)lane] = (uint8_t)k;
                    kt |= k << (2 * e);
                }
                if (f_S) fpt_write_f_words(T, kt, w, lane, f_S, Nreg, NBLK);
                FCD_TRACE(trec, 3);
                return;
            }
            // the vote words are read; the copy below writes other addresses, and its barrier comes before anything else
            if (threadIdx.x == 0) atomicAdd(&dbg->f_sure_fallbacks, 1ull);
        }
    }
    // the r words of the tile's edges: loaded before the barrier so their latency hides behind the staging.
    // Consecutive edges c = n(n-1)/2 + m share n: its words are fetched once per run, not once per edge.
    // Slot numbers (x_u, x_u+1, a_u, a_u+1) of 8 pairs of patients per word, for the edge at hand only: the words of
    // the NEXT edge are requested while this edge's terms run (32 registers less than holding all 8 edges' words).
    uint32_t Zc[NW16], rn[NW16];
    int wn, wm;                          // (n, m) of the edge at hand (wave-uniform walk of the lower-triangular order)
    if (PT) {
        wn = T.cnt0 > 0 ? T.n0 : min(T.n0 + 1, Nreg - 1);      // (a diagonal tile past the last region may draw nothing)
        wm = T.mb;
    } else {
        fcd_edge_to_pair(c0, wn, wm);
    }
    // wave-uniform base + unsigned 32-bit (region, lane) offset: no per-lane 64-bit address arithmetic.  The (up to four)
    // slot words of a region are ONE 16-byte load (ru_index).
    const uint4 *__restrict__ ru = reinterpret_cast<const uint4 *>(r_U) + (int64_t)(w < GW ? w : 0) * Nreg * 64;
    const uint32_t ul = (uint32_t)lane;
    auto comp = [](const uint4 &v, int j) -> uint32_t { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; };
    {
        const uint4 vn = ru[(uint32_t)(wn * 64) + ul], vm = ru[(uint32_t)(wm * 64) + ul];
#pragma unroll
        for (int j = 0; j < NW16; ++j) {
            rn[j] = comp(vn, j);
            const uint32_t rm = comp(vm, j);
            Zc[j] = (rn[j] ^ rm) | ((rn[j] & rm) << 2);
        }
    }
    // S_B of the tile's edges (lane l < 3 of wave e: S_B[c0 + e][l]): asked for HERE, beside the rows -- the build phase turns them
    // into the edge's constants, and a trip to memory in the middle of that phase sat on every tile's critical path
    // (profiles/r04_trace_f.txt: built 3.8 us of a 17 us tile)
    const int wv0 = (int)(threadIdx.x >> 6);
    double sbv = 0.0;
    if (!PRE && wv0 < ne && has(wv0) && lane < 3) sbv = S_B[cid(wv0) * 3 + lane];
    if (PRE) {
        // this wave's edge constants first, then the tile's records: one contiguous piece of the table, coalesced 16-byte
        // copies (two loads per thread in flight); a record's six pieces go to pieces 0-4 and 6 of its 128 bytes in LDS
        const fcd_f_edge_rec *edge_c = reinterpret_cast<const fcd_f_edge_rec *>(frec + (size_t)gridDim.x * NPAIR * (FP_EC * F_REC_PIECES * 16));
        const bool mine = wv0 < FP_EC && has(wv0) && lane == 0;
        fcd_f_edge_rec ek0 = {};
        if (mine) ek0 = edge_c[cid(wv0)];
        const fcd_f4v *src = reinterpret_cast<const fcd_f4v *>(frec) + (size_t)blockIdx.x * NPAIR * (FP_EC * F_REC_PIECES);
        fcd_f4v *dst4 = reinterpret_cast<fcd_f4v *>(ptile);
        const int n16 = NPAIR * (FP_EC * F_REC_PIECES);
        auto at = [](int i) -> int { const int r = i / F_REC_PIECES, k = i - r * F_REC_PIECES; return r * 8 + (k < 5 ? k : 6); };
        for (int i0 = threadIdx.x; i0 < n16; i0 += 2 * blockDim.x) {
            const int i1 = i0 + (int)blockDim.x;
            const fcd_f4v v0 = src[i0], v1 = src[i1 < n16 ? i1 : i0];
            dst4[at(i0)] = v0;
            if (i1 < n16) dst4[at(i1)] = v1;
        }
        // hyper changes from sweep to sweep: the offsets and eta are made here, from the call's constants
        for (int ee = wv0; ee < FP_EC; ee += (int)(blockDim.x >> 6)) {
            if (!has(ee) || lane != 0) continue;
            const fcd_f_edge_rec k = ee == wv0 ? ek0 : edge_c[cid(ee)];
            const double c1 = lg1 + k.d1, c2 = lg2 + k.d2;
            const float cm = fmaxf((float)fabs(c1), (float)fabs(c2)) * 1.0000002f;
            edge_k[ee] = make_float4((float)c1, (float)c2, fcd_draw_f_eta(fcd_f32_sum_err(NPAIR, k.a) + fcd_f32_offset_err(cm, k.a)), 0.f);
        }
    } else if (!PT) {
        // the tile's rows of lMf are one contiguous piece: coalesced 16-byte copies
        const int n_d2 = ne * U * 3;
        const double2 *src = reinterpret_cast<const double2 *>(lMf + c0 * U * 6);
        // (two loads per thread in flight before the first store: a tile is at most 1536 pieces)
        for (int i0 = threadIdx.x; i0 < n_d2; i0 += 2 * blockDim.x) {
            const int i1 = i0 + (int)blockDim.x;
            const double2 v0 = src[i0], v1 = src[i1 < n_d2 ? i1 : i0];
            single[i0] = v0;
            if (i1 < n_d2) single[i1] = v1;
        }
    } else {
        // two contiguous pieces, one per row: row 1's goes to edge slot FT_W
        const int na = T.cnt0 * U * 3, n_d2 = na + T.cnt1 * U * 3, ob = FT_W * U * 3 - na;
        const double2 *sa = reinterpret_cast<const double2 *>(lMf + T.cr0 * U * 6);
        const double2 *sb = reinterpret_cast<const double2 *>(lMf + T.cr1 * U * 6) - na;
        for (int i0 = threadIdx.x; i0 < n_d2; i0 += 2 * blockDim.x) {
            const int i1 = i0 + (int)blockDim.x;
            const int j1 = i1 < n_d2 ? i1 : i0;
            const double2 v0 = i0 < na ? sa[i0] : sb[i0], v1 = j1 < na ? sa[j1] : sb[j1];
            single[i0 < na ? i0 : i0 + ob] = v0;
            if (i1 < n_d2) single[i1 < na ? i1 : i1 + ob] = v1;
        }
    }
    __syncthreads();
    FCD_TRACE(trec, 1);
    if (!PRE) {
        // pair records from the single rows in LDS, ONE THREAD PER (edge, pair): six 16-byte reads (the three mixture cases of
        // patient u and of patient u+1), the nine valid sums, rounded once to fp32, eight 16-byte writes (two slots each; the
        // seven impossible slots -- x and a both set for a patient -- as zeros).  Round 3's build gave every (pair, slot) entry a
        // thread of its own: 16 x the index arithmetic and 7/16 of the threads making zeros -- 3.7 us of a 17 us tile
        // (profiles/r04_trace_f.txt).
        fcd_f4v *dst4 = reinterpret_cast<fcd_f4v *>(ptile);
        const int total = ne * NPAIR;
        // (the records are made by the UPPER half of the workgroup's waves: the lower ones make the edges' bounds below)
        const int half = (int)(blockDim.x >> 7) << 6;
        const int tb = (int)threadIdx.x >= half ? (int)threadIdx.x - half : (int)threadIdx.x + ((int)blockDim.x - half);
        for (int ep = tb; ep < total; ep += blockDim.x) {
            const int e = ep / NPAIR, pr = ep - e * NPAIR;
            if (PT && !has(e)) continue;
            const int u = 2 * pr;
            const double2 *su = single + (e * U + u) * 3;
            double2 A[3], B[3];
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                A[l] = su[l];
                B[l] = (u + 1 < U) ? su[3 + l] : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int s2 = 0; s2 < 8; ++s2) dst4[(pr * FP_EC + e) * 8 + s2] = fp_pair_piece(A, B, s2);       // [pair][edge][slot]: see the reads below
        }
        // the edges' bounds B_e (wave e does edge e, lane = patient; U <= 64)
        for (int ee = (int)(threadIdx.x >> 6); ee < ne; ee += (int)(blockDim.x >> 6)) {      // (a workgroup may have fewer waves than edges)
            if (PT && !has(ee)) continue;
            const float a = fp_edge_bound(single + (ee * U + (lane < U ? lane : 0)) * 3, lane < U);
            if (lane == 0) {
                // the edge's constants as the draw wants them: the two log-odds offsets in fp32 and the relative uncertainty
                // of the weights that the error bound of the whole fp32 sum (NPAIR records, then the offset) amounts to
                const int64_t c = cid(ee);
                double sb0, sb1, sb2;
                if (ee == wv0) {                       // (this wave's own edge: the values asked for at the top)
                    const uint64_t bits = (uint64_t)__double_as_longlong(sbv);      // lane 0 holds S_B[c][0]; lanes 1, 2 the others
                    auto lane_val = [&](int l) -> double {
                        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bits, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(bits >> 32), l);
                        return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
                    };
                    sb0 = lane_val(0); sb1 = lane_val(1); sb2 = lane_val(2);
                } else {
                    sb0 = S_B[c * 3 + 0]; sb1 = S_B[c * 3 + 1]; sb2 = S_B[c * 3 + 2];
                }
                const double c1 = lg1 + (sb1 - sb0), c2 = lg2 + (sb2 - sb0);
                const float cm = fmaxf((float)fabs(c1), (float)fabs(c2)) * 1.0000002f;
                edge_k[ee] = make_float4((float)c1, (float)c2, fcd_draw_f_eta(fcd_f32_sum_err(NPAIR, a) + fcd_f32_offset_err(cm, a)), 0.f);
            }
        }
        __syncthreads();
    }
    FCD_TRACE(trec, 2);
    if (w >= GW) return;
    if (FCD_ABL(0, 3)) return;           // ablation: staging only
#ifdef FCD_ABLATE
    long long tr_terms = 0, tr_draw = 0, tr_rest = 0;
#endif
    const uint32_t chain = chain0 + (uint32_t)w * 64u + lane;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    fcd_u4 rnd = {0, 0, 0, 0};
    int64_t rnd_blk = -1;                // (PT: the Philox block in rnd; a row of the tile may span two)
    uint32_t kt = 0;                     // (PT: the tile's draws, 2 bits per edge)
    const int NG = (NPAIR + 7) >> 3;     // groups of 8 pairs = 16 patients = one slot word
    // The records lie [pair][edge][slot] from LDS address 0 (the kernel declares no static LDS: the host asks the runtime
    // before the first launch), so with the loops over edges, groups and pairs unrolled the record's address is an
    // IMMEDIATE of the read and a term's address costs a shift and a mask -- whatever the number of patients.

#pragma unroll
    for (int e = 0; e < FP_EC; ++e) {
        if (has(e)) {
            const int64_t c = cid(e);
            // next edge: (n, m+1), or (n+1, 0) at the end of row n (clamped past the last edge: unused there)
            int nn = wn, nm = wm + 1;
            if (PT) {
                // PT: (n0 + 1, mb) after the last edge of row n0; clamped to regions that exist (unused there)
                if (e + 1 >= FT_W + (e < FT_W ? 0 : FT_W) || !has(e + 1)) {
                    nn = T.n0 + 1;
                    nm = T.mb;
                }
                nn = nn < Nreg ? nn : Nreg - 1;
                nm = nm < Nreg ? nm : Nreg - 1;
            } else if (nm == nn) {
                nm = 0;
                nn = (nn + 1 < Nreg) ? nn + 1 : nn;
            }
            // the next edge's words: region m always, region n only where the row of the triangle changes (wave-uniform)
            uint4 vmn = make_uint4(0u, 0u, 0u, 0u), vnn = vmn;
            const bool new_row = nn != wn;
            if (e + 1 < FP_EC) {
                vmn = ru[(uint32_t)(nm * 64) + ul];
                if (new_row) vnn = ru[(uint32_t)(nn * 64) + ul];
            }
#ifdef FCD_ABLATE
            const long long tc0 = clock64();
#endif
            fcd_f2v acc = {0.f, 0.f}, acc1 = {0.f, 0.f};    // even / odd pairs: two chains of packed adds, none waits for the one before
#pragma unroll
            for (int g = 0; g < NW16; ++g) {
                if (g < NG) {
                    const uint32_t zs = Zc[g];
                    if (NPAIR - 8 * g >= 8) {
                        // eight reads asked for together, then the eight packed adds
                        fcd_f2v v[8];
#pragma unroll
                        for (int p = 0; p < 8; ++p) {
                            // slot -> 8-byte records: byte offset = slot << 3
                            const uint32_t ad = (p == 0) ? (zs << 3) & 0x78u : (zs >> (4 * p - 3)) & 0x78u;
                            v[p] = *(lds_cf2v *)(uintptr_t)(ad + (uint32_t)(((g * 8 + p) * FP_EC + e) * 128));
                        }
#pragma unroll
                        for (int p = 0; p < 8; p += 2) {
                            if (g == 0 && p == 0) {          // (the sums start from the first terms, not from 0 + the first terms)
                                acc = v[0];
                                acc1 = v[1];
                            } else {
                                acc += v[p];
                                acc1 += v[p + 1];
                            }
                        }
                        __builtin_amdgcn_sched_group_barrier(0x002, 15, 0);     // the addresses (VALU)
                        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);      // the reads (DS read)
                        __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);      // the adds
                    } else {
                        for (int p = 0; p < NPAIR - 8 * g; ++p) {
                            const uint32_t off = ((zs >> (4 * p)) & 15u) << 3;
                            const fcd_f2v v = *(lds_cf2v *)(uintptr_t)(off + (uint32_t)(((g * 8 + p) * FP_EC + e) * 128));
                            acc += v;
                        }
                    }
                }
            }
            acc += acc1;
#ifdef FCD_ABLATE
            asm volatile("" ::"v"(acc.x), "v"(acc.y));
            const long long tc1 = clock64();
#endif
            const float4 ek = edge_k[e];
            if (FCD_ABL(0, 2)) {             // ablation: no RNG / exp
                f_state[((int64_t)w * C + c) * 64 + lane] = (uint8_t)(acc.x > acc.y ? 1 : 2);
                continue;
            }
            uint32_t xw;
            if (!PT) {
                if ((e & 3) == 0) rnd = fcd_philox((uint32_t)(c >> 2), chain, sweep, FCD_KIND_F, k0, k1);   // c0 is a multiple of 8
                xw = fcd_word(rnd, e & 3);
            } else {
                if ((c >> 2) != rnd_blk) {
                    rnd_blk = c >> 2;
                    rnd = fcd_philox((uint32_t)rnd_blk, chain, sweep, FCD_KIND_F, k0, k1);
                }
                xw = fcd_word(rnd, (int)(c & 3));
            }
            bool amb = false;
            int k;
            const float bf1 = ek.x + acc.x, bf2 = ek.y + acc.y, xf = (float)xw * 2.3283064e-10f;
            // (no exponential where the mode leads by more than e^15 in every lane -- the usual case on separated data -- unless
            // the test hook f_tol asks for the exact path everywhere)
            if (margin > 1.f || __ballot(!fcd_draw_f_sure(bf1, bf2, xf, ek.z, &k)) != 0ull) k = fcd_draw_f_fast32(bf1, bf2, xf, ek.z, margin, &amb);
            if (__ballot(amb) != 0ull) {
                // somewhere in the wave the fp32 sums cannot decide the draw: the edge again, in fp64, for the whole wave
                k = fcd_f_exact_edge(lMf + c * U * 6, lg1 + (S_B[c * 3 + 1] - S_B[c * 3 + 0]), lg2 + (S_B[c * 3 + 2] - S_B[c * 3 + 0]), Zc[0],
                                     NW16 > 1 ? Zc[NW16 > 1 ? 1 : 0] : 0u, NW16 > 2 ? Zc[NW16 > 2 ? 2 : 0] : 0u, NW16 > 3 ? Zc[NW16 > 3 ? 3 : 0] : 0u, U, xw);
                kt |= (uint32_t)(k >> 2) << (16 + e);       // (FCD_F_OPEN: this lane's draw of edge e is made again behind the loop)
                k &= 3;
                if (lane == 0) atomicAdd(&dbg->f_repeats, 1ull);
            }
#ifdef FCD_ABLATE
            asm volatile("" ::"v"(k));
            const long long tc2 = clock64();
#endif
            (f_state + ((int64_t)w * C + c) * 64)[(uint32_t)lane] = (uint8_t)k;     // (scalar base + lane)
            if (PT) kt |= (uint32_t)k << (2 * e);
            if (!PT && fsq) {
                // square copy for the r pass that follows (fcd_gibbs_sweeps): rows of it are contiguous in m
                uint8_t *sq = fsq + (int64_t)w * Nreg * Nreg * 64;
                (sq + ((int64_t)wn * Nreg + wm) * 64)[(uint32_t)lane] = (uint8_t)k;
                (sq + ((int64_t)wm * Nreg + wn) * 64)[(uint32_t)lane] = (uint8_t)k;
            }
            if (e + 1 < FP_EC) {
#pragma unroll
                for (int j = 0; j < NW16; ++j) {
                    if (new_row) rn[j] = comp(vnn, j);
                    const uint32_t rm = comp(vmn, j);
                    Zc[j] = (rn[j] ^ rm) | ((rn[j] & rm) << 2);
                }
                wn = nn;
                wm = nm;
            }
#ifdef FCD_ABLATE
            {
                asm volatile("" ::"v"(Zc[0]));
                const long long tc3 = clock64();
                tr_terms += tc1 - tc0;
                tr_draw += tc2 - tc1;
                tr_rest += tc3 - tc2;
            }
#endif
        }
    }
    if (__builtin_expect(__ballot(kt >> 16) != 0ull, 0)) {
        // some lane's log-odds of some edge were not finite (type 0 impossible there): those draws again, from the absolute
        // log-weights -- never on finite tables with positive gamma.  On the call's record table (PRE) lM and hyper are read from
        // the device words gibbs_f_hint_kernel left them in, not from the arguments: a value that has to live to the end of the kernel
        // costs every wave scalar moves in its prologue (the decided-tile path is little else), and dbg lives that long anyway.
        const double *__restrict__ lMa = PRE ? dbg->lM : lM;
        const double *__restrict__ hya = PRE ? dbg->hyper : hyper;
#pragma unroll 1
        for (int e = 0; e < FP_EC; ++e) {
            const bool open = (kt >> (16 + e)) & 1u;
            if (__ballot(open) == 0ull) continue;
            const int64_t c = cid(e);
            int n, m;
            if (PT) {
                n = T.n0 + (e < FT_W ? 0 : 1);
                m = T.mb + e % FT_W;
            } else {
                fcd_edge_to_pair(c, n, m);
            }
            const uint32_t ka = (uint32_t)fcd_f_abs_edge(lMa, S_B, hya, ru, c, n, m, U, chain, sweep, seed);
            if (open) {
                kt = (kt & ~(3u << (2 * e))) | (ka << (2 * e));
                (f_state + ((int64_t)w * C + c) * 64)[(uint32_t)lane] = (uint8_t)ka;
                if (!PT && fsq) {
                    uint8_t *sq = fsq + (int64_t)w * Nreg * Nreg * 64;
                    (sq + ((int64_t)n * Nreg + m) * 64)[(uint32_t)lane] = (uint8_t)ka;
                    (sq + ((int64_t)m * Nreg + n) * 64)[(uint32_t)lane] = (uint8_t)ka;
                }
            }
        }
    }
    if (PT && f_S) fpt_write_f_words(T, kt, w, lane, f_S, Nreg, NBLK);
#ifdef FCD_ABLATE
    FCD_TRACE_VAL(trec, 4, tr_terms);
    FCD_TRACE_VAL(trec, 5, tr_draw);
    FCD_TRACE_VAL(trec, 6, tr_rest);
#endif
    FCD_TRACE(trec, 3);
}

// What the build phase of a pair-aligned tile makes depends on lMf and S_B alone, and neither can change inside one call of
// the sweep loop: this kernel makes it for every tile of the call at once -- workgroup = tile, the same sums, the same bound
// (wave e = edge e, lane = patient, fp_edge_bound) -- and gibbs_f_pair_kernel<.., true, true> copies it.  Layout: see PRE.
// Pieces of edges the tile does not hold (past the diagonal) are never written and never read.
// It also leaves every edge's bounds for the rule of decided edges (fcd_f_edge_mode) and, where some tile has all its edges
// decided at the call's starting hyper with FCD_F_SURE_DRIFT nats in hand, a 1 in dbg->tile_decided: a table without such a tile is
// read by the kernel without the decided-tile path.
__global__ __launch_bounds__(64 * FP_EC) void gibbs_f_records_kernel(const double *__restrict__ S_B, const double *__restrict__ lMf,
                                                                     const double *__restrict__ hyper, int Nreg, int U,
                                                                     char *__restrict__ frec, fcd_dev_words *__restrict__ dbg,
                                                                     unsigned *__restrict__ votes, int n_votes) {
    const int NPAIR = (U + 1) >> 1;
    const fpt_tile T = fpt_locate((int)blockIdx.x, Nreg);
    // (the run kernel's vote words: zero before the call's first pass; every pass leaves them zero)
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n_votes; i += (int)(gridDim.x * blockDim.x)) votes[i] = 0u;
    auto has = [&](int e) -> bool { return (e % FT_W) < (e < FT_W ? T.cnt0 : T.cnt1); };
    auto cid = [&](int e) -> int64_t { return (e < FT_W ? T.cr0 : T.cr1) + (e % FT_W); };
    fcd_f4v *dst4 = reinterpret_cast<fcd_f4v *>(frec) + (size_t)blockIdx.x * NPAIR * (FP_EC * F_REC_PIECES);
    // one thread per (edge, pair), the pairs of an edge side by side: its two patients' rows are 96 contiguous bytes
    for (int ep = threadIdx.x; ep < FP_EC * NPAIR; ep += blockDim.x) {
        const int e = ep / NPAIR, pr = ep - e * NPAIR;
        if (!has(e)) continue;
        const int u = 2 * pr;
        const double2 *su = reinterpret_cast<const double2 *>(lMf + cid(e) * U * 6) + u * 3;
        double2 A[3], B[3];
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            A[l] = su[l];
            B[l] = (u + 1 < U) ? su[3 + l] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2)
            if (s2 != 5 && s2 != 7) dst4[(pr * FP_EC + e) * F_REC_PIECES + (s2 < 5 ? s2 : 5)] = fp_pair_piece(A, B, s2);
    }
    const int e = (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    __shared__ int open_edges;       // edges of the tile that the hint's rule leaves open
    if (threadIdx.x == 0) open_edges = 0;
    __syncthreads();
    if (has(e)) {                // (wave-uniform)
        const int64_t c = cid(e);
        const double2 *su = reinterpret_cast<const double2 *>(lMf + c * U * 6) + (lane < U ? lane : 0) * 3;
        const float a = fp_edge_bound(su, lane < U);
        // the six bounds of fcd_f_edge_mode: this patient's smallest and largest d_1, d_2 and d_1 - d_2 over the three cases
        double b[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        bool finite = true;
        if (lane < U) {
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                const double v[3] = {su[l].x, su[l].y, su[l].x - su[l].y};
                finite = finite && isfinite(v[0]) && isfinite(v[1]);
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    b[2 * q] = l == 0 ? v[q] : fmin(b[2 * q], v[q]);
                    b[2 * q + 1] = l == 0 ? v[q] : fmax(b[2 * q + 1], v[q]);
                }
            }
        }
        finite = __ballot(!finite) == 0ull;
#pragma unroll
        for (int q = 0; q < 6; ++q) b[q] = fcd_wave_sum(b[q]);
        if (lane == 0) {
            fcd_f_edge_rec k = {};
            const double sb0 = S_B[c * 3 + 0];
            k.d1 = S_B[c * 3 + 1] - sb0;
            k.d2 = S_B[c * 3 + 2] - sb0;
            k.a = a;
            // outward: the wave's sums of up to 64 terms are off by at most 6 x 2^-53 x sum |term| <= 1.4e-15 a (|d_1 - d_2| <= twice
            // the row's largest |entry|, and its own rounding), then the conversions round away from the interval
            const double slack = 8e-15 * (double)a;
#pragma unroll
            for (int q = 0; q < 6; ++q)
                k.b[q] = !finite ? __builtin_nanf("") : (q & 1) ? __double2float_ru(b[q] + slack) : __double2float_rd(b[q] - slack);
            reinterpret_cast<fcd_f_edge_rec *>(frec + (size_t)gridDim.x * NPAIR * (FP_EC * F_REC_PIECES * 16))[c] = k;
            const double c1 = (hyper[FCD_H_LNGAMMA + 1] - hyper[FCD_H_LNGAMMA + 0]) + k.d1;
            const double c2 = (hyper[FCD_H_LNGAMMA + 2] - hyper[FCD_H_LNGAMMA + 0]) + k.d2;
            if (fcd_f_edge_mode(c1, c2, k.b, fcd_f_edge_delta(c1, c2, NPAIR, a), FCD_F_SURE_T - FCD_F_SURE_DRIFT) < 0) open_edges = 1;
        }
    }
    __syncthreads();
    // (every tile that has the property stores the same word: no atomic, no fence -- gibbs_f_hint_kernel reads it behind
    // this launch)
    // ... and every tile that lacks it stores a 1 into the word beside it: "some tile is open"
    if (threadIdx.x == 0 && (T.cnt0 > 0 || T.cnt1 > 0)) *(open_edges ? &dbg->tile_open : &dbg->tile_decided) = 1u;
}
// ... and hands it to the host: 4 build + 2 all + any into the pinned word the sweep loop polls (written once, complete; all =
// some tile is decided and none is open), the device words cleared for the next build.
// It also leaves the call's lM and hyper where the kernels that read the table find them (dbg->lM, dbg->hyper).
__global__ void gibbs_f_hint_kernel(fcd_dev_words *__restrict__ dbg, volatile unsigned *hint, unsigned build, const double *lM,
                                    const double *hyper) {
    const unsigned any = dbg->tile_decided != 0u ? 1u : 0u, all = (any && dbg->tile_open == 0u) ? 1u : 0u;
    dbg->tile_decided = 0u;
    dbg->tile_open = 0u;
    dbg->lM = lM;
    dbg->hyper = hyper;
    // ... and the starting hyper itself for the r pass's bound build, which runs after the first M-step
    for (int i = 0; i < 5; ++i) dbg->hyper0[i] = hyper[i];
    __hip_atomic_store(const_cast<unsigned *>(hint), 4u * build + 2u * all + any, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------------------------
// The decided path in block-wide runs (fpr_run, fcd_common.h): work item = (run, chain word), one wave; workgroup = the run
// x the (up to) FR_WAVES = 8 chain words of blockIdx.y.  No LDS image, no barrier before the stores, and no tile ever goes
// back as a whole: lane e < 32 evaluates edge e's rule once per run, every lane draws the run's Philox blocks once per row
// (a tile's two rows of four ids straddle 3.45 blocks, a run's two rows of sixteen 8.9 for up to four tiles) and tests the
// words of the present edges against fcd_draw_f_sure's range.  An edge the rule leaves open, or for which some lane of THIS wave is out of
// range, is drawn by this wave as gibbs_f_pair_kernel draws it (fcd_f_run_edge); every other edge gets its mode, which is
// what that kernel gives every (wave, edge) without an out-of-range lane, on either of its paths.
// Given slots or cnt_f it also counts what it stores -- the f half of the sweep's tally (knob tally_in_f; DESIGN.md, "The f
// counts in the run kernel"): with both null it does what it did before.
// ---------------------------------------------------------------------------------------------
// One edge's draw for the whole wave, as the term loop of gibbs_f_pair_kernel and what follows it make it: the fp32 sums in
// that loop's order (full groups of eight pairs: even pairs into acc, odd pairs into acc1, the sums starting from the first
// terms; a short last group into acc; then acc += acc1), from the call's record table in global memory
// (rec: the edge's record of pair 0; a record is F_REC_PIECES 16-byte pieces, pair p lies p * FP_EC records on; Z: the slot
// words of the edge's two regions).  Returns the draw, + FPR_AMB where some lane of the wave asks for the exact path: the
// kernel calls that itself, so that this function calls none and needs no stack.
constexpr int FPR_AMB = 8;
__device__ __attribute__((noinline)) int fcd_f_run_edge(const char *__restrict__ rec, const fcd_f_edge_rec *__restrict__ ke_p,
                                                        const double *__restrict__ hyper, uint4 Z, int U, uint32_t xw, float margin) {
    const int NPAIR = (U + 1) >> 1, NG = (NPAIR + 7) >> 3;
    auto term = [&](int p, uint32_t slot) -> fcd_f2v {
        const uint32_t s2 = slot >> 1;
        return *reinterpret_cast<const fcd_f2v *>(rec + (size_t)p * (FP_EC * F_REC_PIECES * 16) + (s2 < 5 ? s2 : 5) * 16 + (slot & 1u) * 8);
    };
    fcd_f2v acc = {0.f, 0.f}, acc1 = {0.f, 0.f};
#pragma unroll 1
    for (int g = 0; g < NG; ++g) {
        const uint32_t zs = g == 0 ? Z.x : g == 1 ? Z.y : g == 2 ? Z.z : Z.w;
        const int np = NPAIR - 8 * g;
        if (np >= 8) {
#pragma unroll 1
            for (int p = 0; p < 8; p += 2) {
                const fcd_f2v v0 = term(8 * g + p, (zs >> (4 * p)) & 15u), v1 = term(8 * g + p + 1, (zs >> (4 * p + 4)) & 15u);
                if (g == 0 && p == 0) {
                    acc = v0;
                    acc1 = v1;
                } else {
                    acc += v0;
                    acc1 += v1;
                }
            }
        } else {
#pragma unroll 1
            for (int p = 0; p < np; ++p) acc += term(8 * g + p, (zs >> (4 * p)) & 15u);
        }
    }
    acc += acc1;
    const fcd_f_edge_rec ke = *ke_p;
    const double lg1 = hyper[FCD_H_LNGAMMA + 1] - hyper[FCD_H_LNGAMMA + 0], lg2 = hyper[FCD_H_LNGAMMA + 2] - hyper[FCD_H_LNGAMMA + 0];
    const double c1 = lg1 + ke.d1, c2 = lg2 + ke.d2;
    const float cm = fmaxf((float)fabs(c1), (float)fabs(c2)) * 1.0000002f;
    const float eta = fcd_draw_f_eta(fcd_f32_sum_err(NPAIR, ke.a) + fcd_f32_offset_err(cm, ke.a));
    const float bf1 = (float)c1 + acc.x, bf2 = (float)c2 + acc.y, xf = (float)xw * 2.3283064e-10f;
    bool amb = false;
    int k;
    if (margin > 1.f || __ballot(!fcd_draw_f_sure(bf1, bf2, xf, eta, &k)) != 0ull) k = fcd_draw_f_fast32(bf1, bf2, xf, eta, margin, &amb);
    return k | (__ballot(amb) != 0ull ? FPR_AMB : 0);
}

// the two-bit fields 2j of x <- bit j of m (j < 16)
__device__ __forceinline__ uint32_t fpr_spread16(uint32_t m) {
    m = (m | (m << 8)) & 0x00FF00FFu;
    m = (m | (m << 4)) & 0x0F0F0F0Fu;
    m = (m | (m << 2)) & 0x33333333u;
    return (m | (m << 1)) & 0x55555555u;
}
// the r pass's eight f bytes of one (row, block) from the row's sixteen draws (2 bits per column): byte p = (3 f(2p) + f(2p + 1)) << 2
__device__ __forceinline__ uint2 fpr_row_word(uint32_t K) {
    const uint32_t v = 3u * (K & 0x33333333u) + ((K >> 2) & 0x33333333u);      // nibble p: 3 f(2p) + f(2p + 1) <= 8
    uint32_t lo = v & 0xFFFFu, hi = v >> 16;
    lo = (lo | (lo << 8)) & 0x00FF00FFu;
    hi = (hi | (hi << 8)) & 0x00FF00FFu;
    lo = (lo | (lo << 4)) & 0x0F0F0F0Fu;
    hi = (hi | (hi << 4)) & 0x0F0F0F0Fu;
    return make_uint2(lo << 2, hi << 2);
}

__global__ __launch_bounds__(64 * FR_WAVES) void gibbs_f_run_kernel(const double *__restrict__ S_B, const double *__restrict__ lMf,
                                                           const double *__restrict__ hyper, uint8_t *__restrict__ f_state,
                                                           const uint32_t *__restrict__ r_U, int Nreg, int U, int64_t C, int GW,
                                                           uint32_t chain0, uint64_t seed, uint32_t sweep, float margin,
                                                           uint2 *__restrict__ f_S, int NBLK, fcd_dev_words *__restrict__ dbg,
                                                           const char *__restrict__ frec, const double *__restrict__ lM, int n_tiles,
                                                           unsigned *__restrict__ votes, int64_t G,
                                                           unsigned long long *__restrict__ slots, uint32_t *__restrict__ cnt_f) {
    static_assert(16 % FR_WAVES == 0, "a workgroup's chain words lie in one group of 16");
    static_assert(FR_W == R_NB && FR_W == 16 && FT_W == 4, "a run is one block of the r pass's f words: sixteen columns, four tiles");
    __shared__ uint32_t vote[FR_WAVES];  // per wave: the run's tiles (bit q) in which some lane's uniform is out of range
    // per wave and edge (slots or cnt_f given: this launch counts f, the f half of the sweep's tally): the edge's ones | twos << 16
    // over the wave's valid chains -- at most 64 each
    __shared__ uint32_t pairs[FR_WAVES][2 * FR_W];
    const bool counting = slots != nullptr || cnt_f != nullptr;       // (kernel arguments: wave-uniform)
    const int NPAIR = (U + 1) >> 1;
    const fpr_run R = fpr_locate((int)blockIdx.x, Nreg);
    const int lane = threadIdx.x & 63;
    const int wv = (int)(threadIdx.x >> 6);
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * (blockDim.x >> 6)) + wv);
    const size_t rec_tile = (size_t)NPAIR * (FP_EC * F_REC_PIECES * 16);        // bytes of a tile's records
    const fcd_f_edge_rec *edge_c = reinterpret_cast<const fcd_f_edge_rec *>(frec + (size_t)n_tiles * rec_tile);
    // lane e < 32: edge e's rule at this sweep's hyper
    const int lr = (lane >> 4) & 1, lj = lane & (FR_W - 1);
    const bool present = lane < 2 * FR_W && lj < (lr ? R.cnt1 : R.cnt0);
    int mode = -1;
    if (present) {
        const fcd_f_edge_rec k = edge_c[(lr ? R.cr1 : R.cr0) + lj];
        const double c1 = (hyper[FCD_H_LNGAMMA + 1] - hyper[FCD_H_LNGAMMA + 0]) + k.d1;
        const double c2 = (hyper[FCD_H_LNGAMMA + 2] - hyper[FCD_H_LNGAMMA + 0]) + k.d2;
        mode = fcd_f_edge_mode(c1, c2, k.b, fcd_f_edge_delta(c1, c2, NPAIR, k.a), FCD_F_SURE_T);
    }
    const uint32_t pm = (uint32_t)__ballot(present), dm = (uint32_t)__ballot(mode >= 0);
    const uint32_t m1 = (uint32_t)__ballot(mode == 1), m2 = (uint32_t)__ballot(mode == 2);
    uint32_t oe = 0;                     // edges for which some lane of this wave is out of range (wave-uniform)
    if (w < GW) {
        const uint32_t chain = chain0 + (uint32_t)w * 64u + lane;
        uint32_t out = 0;                // this lane's
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int cnt = r ? R.cnt1 : R.cnt0;
            if (cnt == 0) continue;
            const int64_t cr = r ? R.cr1 : R.cr0;
            const int64_t b1 = (cr + cnt - 1) >> 2;
#pragma unroll 1
            for (int64_t b = cr >> 2; b <= b1; ++b) {
                const fcd_u4 rnd = fcd_philox((uint32_t)b, chain, sweep, FCD_KIND_F, (uint32_t)seed, (uint32_t)(seed >> 32));
                const int j0 = (int)(4 * b - cr);        // column (from the run's first) of the block's word 0
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float xf = (float)fcd_word(rnd, q) * 2.3283064e-10f;
                    const bool bad = !(xf > 1e-6f && xf < 0.999999f);
                    if (bad && j0 + q >= 0 && j0 + q < cnt) out |= 1u << (FR_W * r + j0 + q);
                }
            }
        }
        if (__ballot(out != 0u) != 0ull) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) out |= (uint32_t)__shfl_xor((int)out, o, 64);
            oe = (uint32_t)__builtin_amdgcn_readfirstlane((int)out);
        }
        // the draws, 2 bits per column: the modes, then this wave's own draws of its exceptional edges
        uint32_t K0 = (fpr_spread16(m1 & 0xFFFFu) | (fpr_spread16(m2 & 0xFFFFu) << 1));
        uint32_t K1 = (fpr_spread16(m1 >> 16) | (fpr_spread16(m2 >> 16) << 1));
        const uint32_t X = (pm & ~dm) | oe;
        if (__builtin_expect(X != 0u, 0)) {
            const uint4 *__restrict__ ru = reinterpret_cast<const uint4 *>(r_U) + (int64_t)w * Nreg * 64;
            uint32_t x = X;
#pragma unroll 1
            while (x != 0u) {
                const int e = __builtin_ctz(x);
                x &= x - 1u;
                const int r = e >> 4, j = e & (FR_W - 1);
                const int64_t c = (r ? R.cr1 : R.cr0) + j;
                // the edge's record: tile tile0 + j / FT_W, edge (r, j % FT_W) of it
                const char *rec = frec + (size_t)(R.tile0 + j / FT_W) * rec_tile + (size_t)(r * FT_W + j % FT_W) * (F_REC_PIECES * 16);
                const fcd_u4 rnd = fcd_philox((uint32_t)(c >> 2), chain, sweep, FCD_KIND_F, (uint32_t)seed, (uint32_t)(seed >> 32));
                const uint32_t xw = fcd_word(rnd, (int)(c & 3));
                const int n = R.n0 + r, m = R.mb + j;
                const uint4 vn = ru[(uint32_t)(n * 64) + (uint32_t)lane], vm = ru[(uint32_t)(m * 64) + (uint32_t)lane];
                const uint4 Z = make_uint4((vn.x ^ vm.x) | ((vn.x & vm.x) << 2), (vn.y ^ vm.y) | ((vn.y & vm.y) << 2),
                                           (vn.z ^ vm.z) | ((vn.z & vm.z) << 2), (vn.w ^ vm.w) | ((vn.w & vm.w) << 2));
                uint32_t k = (uint32_t)fcd_f_run_edge(rec, edge_c + c, hyper, Z, U, xw, margin);
                if (k & FPR_AMB) {
                    // somewhere in the wave the fp32 sums cannot decide the draw: the edge again, in fp64, for the whole wave
                    const double lg1 = hyper[FCD_H_LNGAMMA + 1] - hyper[FCD_H_LNGAMMA + 0], lg2 = hyper[FCD_H_LNGAMMA + 2] - hyper[FCD_H_LNGAMMA + 0];
                    k = (uint32_t)fcd_f_exact_edge(lMf + c * U * 6, lg1 + (S_B[c * 3 + 1] - S_B[c * 3 + 0]), lg2 + (S_B[c * 3 + 2] - S_B[c * 3 + 0]),
                                                   Z.x, Z.y, Z.z, Z.w, U, xw);
                    if (lane == 0) atomicAdd(&dbg->f_repeats, 1ull);
                    const bool open = (k & FCD_F_OPEN) != 0;
                    k &= 3u;
                    if (__ballot(open) != 0ull) {
                        const uint32_t ka = (uint32_t)fcd_f_abs_edge(lM, S_B, hyper, ru, c, n, m, U, chain, sweep, seed);
                        if (open) k = ka;
                    }
                }
                if (r) K1 = (K1 & ~(3u << (2 * j))) | (k << (2 * j));
                else K0 = (K0 & ~(3u << (2 * j))) | (k << (2 * j));
            }
        }
        if (counting) {
            // The f half of the tally, from what this wave is about to store: an edge outside X has its mode in every lane,
            // so its count is the word's valid chains on the side the mode names -- wave-uniform numbers, no ballot; an edge
            // of X has per-lane draws, final in K0 / K1 (after the fp64 repeat and the open-edge draw), and is counted
            // there.  Lane e < 32 takes edge e's pair.
            const uint64_t act = fcd_active_mask(w, G);
            const uint32_t nvalid = (uint32_t)__popcll(act);
            uint32_t pair = 0;
            if (lane < 2 * FR_W) pair = ((m1 >> lane) & 1u) ? nvalid : (((m2 >> lane) & 1u) ? nvalid << 16 : 0u);
            uint32_t x = X;
#pragma unroll 1
            while (x != 0u) {
                const int e = __builtin_ctz(x);
                x &= x - 1u;
                const uint32_t k = (((e >> 4) ? K1 : K0) >> (2 * (e & (FR_W - 1)))) & 3u;
                const uint32_t n1 = (uint32_t)__popcll(__ballot(k == 1u) & act), n2 = (uint32_t)__popcll(__ballot(k == 2u) & act);
                if (lane == e) pair = n1 | (n2 << 16);
            }
            if (lane < 2 * FR_W) pairs[wv][lane] = pair;
        }
        // f_state: the edges of a row are consecutive 64-byte lines.  A row without an exceptional edge: lane l writes 16 bytes
        // of edge l / 4 (its mode in every chain), one store; any other row edge by edge, a byte per lane.
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int cnt = r ? R.cnt1 : R.cnt0;
            if (cnt == 0) continue;
            uint8_t *line = f_state + ((int64_t)w * C + (r ? R.cr1 : R.cr0)) * 64;
            const uint32_t Kr = r ? K1 : K0;
            if (((X >> (FR_W * r)) & 0xFFFFu) == 0u) {
                if ((lane >> 2) < cnt) {
                    const uint32_t v = ((Kr >> (2 * (lane >> 2))) & 3u) * 0x01010101u;
                    reinterpret_cast<uint4 *>(line)[lane] = make_uint4(v, v, v, v);
                }
            } else {
#pragma unroll 1
                for (int j = 0; j < cnt; ++j) (line + j * 64)[(uint32_t)lane] = (uint8_t)((Kr >> (2 * j)) & 3u);
            }
        }
        if (f_S) {
            // the r pass's f words.  A full run (sixteen columns below the diagonal pair or up to it): the eight bytes of each
            // row's (n, block) word in one store; column halves and zeros tile by tile.  Any other run: tile by tile.
            const bool full = R.n0 + 2 - R.mb >= FR_W;
            if (full) {
                // (the diagonal pair of row n0: (n0, n0 + 1) is the edge (n0 + 1, n0) of row 1)
                const int jd = R.n0 + 1 - R.mb;
                const uint32_t K0d = jd < FR_W ? K0 | (((K1 >> (2 * (jd - 1))) & 3u) << (2 * jd)) : K0;
                uint2 *word = f_S + (int64_t)w * Nreg * NBLK * 64 + lane;
                word[(int64_t)(R.n0 * NBLK + R.mb / R_NB) * 64] = fpr_row_word(K0d);
                if (R.n0 + 1 < Nreg) word[(int64_t)((R.n0 + 1) * NBLK + R.mb / R_NB) * 64] = fpr_row_word(K1);
            }
#pragma unroll 1
            for (int q = 0; q < R.ntile; ++q) {
                fpt_tile T;
                T.n0 = R.n0;
                T.mb = R.mb + FT_W * q;
                T.cnt0 = min(FT_W, T.n0 - T.mb);
                T.cnt1 = T.n0 + 1 < Nreg ? min(FT_W, T.n0 + 1 - T.mb) : 0;
                T.cr0 = R.cr0 + FT_W * q;
                T.cr1 = R.cr1 + FT_W * q;
                const uint32_t kt = ((K0 >> (8 * q)) & 0xFFu) | (((K1 >> (8 * q)) & 0xFFu) << 8);
                if (full) fpt_write_f_words<false>(T, kt, w, lane, f_S, Nreg, NBLK);
                else fpt_write_f_words<true>(T, kt, w, lane, f_S, Nreg, NBLK);
            }
        }
    }
    // the counters keep their meaning: per (pair-aligned tile, group of 16 chain words) with every present edge decided,
    // f_sure_tiles where no lane of the group is out of range, f_sure_fallbacks where one is -- one word per wave, one barrier
    // BEHIND the stores; the (up to 16 / FR_WAVES) workgroups of a group then meet in the item's word of the record table: each
    // adds 1 << 16 and its tiles in a nibble of its own, the last one counts and leaves the word zero for the next pass
    uint32_t ot = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (oe & (0x000F000Fu << (FT_W * q))) ot |= 1u << q;
    if (lane == 0) vote[wv] = ot;
    __syncthreads();
    if (counting && wv == (int)(blockDim.x >> 6) - 1) {
        // the waves' rows summed, one edge per lane (the workgroup's last wave: the first has the votes); the workgroups of
        // the other chain words meet the same edges, so the counters take atomic adds -- none returns, none adds zero
        const int w0 = (int)(blockIdx.y * (blockDim.x >> 6));
        const int nwv = min((int)(blockDim.x >> 6), GW - w0);              // waves that hold a chain word (their rows are written)
        const int64_t rem = G - (int64_t)w0 * 64;
        const uint32_t nv = (uint32_t)(rem < (int64_t)nwv * 64 ? rem : (int64_t)nwv * 64);      // their valid chains
        uint32_t sum = 0;
        if (present)
            for (int q = 0; q < nwv; ++q) sum += pairs[q][lane];        // (each half at most 8 x 64)
        const uint32_t ones = sum & 0xFFFFu, twos = sum >> 16;
        if (cnt_f && present) {
            uint32_t *ctr = cnt_f + ((lr ? R.cr1 : R.cr0) + lj) * 3;
            const uint32_t zeros = nv - ones - twos;
            if (zeros) (void)__hip_atomic_fetch_add(ctr + 0, zeros, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ones) (void)__hip_atomic_fetch_add(ctr + 1, ones, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (twos) (void)__hip_atomic_fetch_add(ctr + 2, twos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (slots) {
            // the pooled totals (zeros, ones, twos over the present edges: what fcd_tally_f_block adds to acc[1..3]) go to
            // one of FCD_F_SLOTS lines, one atomic each per workgroup; a wave of the r pass behind this launch folds the
            // lines into acc (fcd_f_slots_fold).  32 edges x 512: both halves stay below 2^16
            uint32_t tot = sum;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) tot += (uint32_t)__shfl_xor((int)tot, o, 64);
            if (lane == 0) {
                unsigned long long *line = slots + ((blockIdx.x + 29u * blockIdx.y) & (FCD_F_SLOTS - 1)) * 8;
                const unsigned long long t1 = tot & 0xFFFFu, t2 = tot >> 16;
                const unsigned long long t0 = (unsigned long long)__popc(pm) * nv - t1 - t2;
                if (t0) (void)__hip_atomic_fetch_add(line + 0, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (t1) (void)__hip_atomic_fetch_add(line + 1, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (t2) (void)__hip_atomic_fetch_add(line + 2, t2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (wv == 0) {
        const uint32_t v = lane < (int)(blockDim.x >> 6) ? vote[lane & (FR_WAVES - 1)] : 0u;
        uint32_t bm = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (__ballot((v >> q) & 1u) != 0ull) bm |= 1u << q;
        // the group's workgroups: its chain words [16 y, min(16 y + 16, GW)) in pieces of blockDim.x / 64
        const int w0 = (int)(blockIdx.y * (blockDim.x >> 6)), wpg = (int)(blockDim.x >> 6);
        const int n_wg = (min(16, GW - (w0 & ~15)) + wpg - 1) / wpg;
        bool last = true;
        if (n_wg > 1) {
            uint32_t all = 0;
            if (lane == 0) {
                unsigned *word = votes + (size_t)blockIdx.x * (size_t)((GW + 15) >> 4) + (size_t)(w0 >> 4);
                const uint32_t mine = 0x10000u | (bm << (4 * ((w0 & 15) / wpg)));
                all = atomicAdd(word, mine) + mine;
                if ((int)(all >> 16) == n_wg) atomicExch(word, 0u);
            }
            all = (uint32_t)__builtin_amdgcn_readfirstlane((int)all);
            last = (int)(all >> 16) == n_wg;
            bm = (all | (all >> 4) | (all >> 8) | (all >> 12)) & 15u;
        }
        uint32_t n_sure = 0, n_back = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t tm = (0x000F000Fu << (FT_W * q)) & pm;
            if (last && tm != 0u && (tm & ~dm) == 0u) {
                if ((bm >> q) & 1u) n_back += 1;
                else n_sure += 1;
            }
        }
        if (lane == 0) {
            if (n_sure) atomicAdd(&dbg->f_sure_tiles, (unsigned long long)n_sure);
            if (n_back) atomicAdd(&dbg->f_sure_fallbacks, (unsigned long long)n_back);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// f step, pair form for ANY number of patients (what cfg5's U = 250 runs).  Same records, same term (one
// ds_read_b128 + two fp64 adds per PAIR of patients), but
//   * the tile holds EC edges with EC chosen by the host so that two workgroups share a CU (EC * NPAIR * 256 B <= 80 KiB),
//   * the pair records are built from 384-byte pieces of the rows that each wave stages in a small LDS scratch of its
//     own (no whole single rows in LDS: at U = 250 they would cost 12 KB per edge), every table byte loaded once,
//   * the slot words of a group of 16 patients are loaded per group, one group ahead (a wave cannot hold the
//     16 words per region that U = 250 needs), the group loop is a run-time loop.
// One Philox block still serves four edges; a tile of EC < 4 edges recomputes it (c0 is a multiple of EC, EC | 4).
// ---------------------------------------------------------------------------------------------
template <int EC>
__global__ __launch_bounds__(1024, 8) void gibbs_f_pairx_kernel(const double *__restrict__ S_B, const double *__restrict__ lMf,
                                                                const double *__restrict__ hyper, uint8_t *__restrict__ f_state,
                                                                const uint32_t *__restrict__ r_U, int Nreg, int U, int64_t C,
                                                                int GW, uint32_t chain0, uint64_t seed, uint32_t sweep,
                                                                float margin, uint8_t *__restrict__ fsq,
                                                                fcd_dev_words *__restrict__ dbg, const double *__restrict__ lM) {
    // pairs [EC][NPAIR][16] float2 | per-edge constants [8] float4 | staging scratch [waves][2][24] double2
    extern __shared__ __attribute__((aligned(256))) double ptile[];
    const int NPAIR = (U + 1) >> 1, NW16 = (U + 15) >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * EC;
    const int ne = (int)((C - c0 < EC) ? (C - c0) : EC);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    int wn, wm;                          // (n, m) of the edge at hand (wave-uniform walk of the lower-triangular order)
    fcd_edge_to_pair(c0, wn, wm);
    const uint32_t *__restrict__ ru = r_U + (int64_t)(w < GW ? w : 0) * Nreg * (NW16 <= 4 ? 4 : NW16) * 64;
    const uint32_t ul = (uint32_t)lane;
    // slot words of the first group of the first edge: requested before the build so that their latency hides behind it
    // (slot word g of region n for this lane: [word][lane], or -- up to four words, forced onto this kernel by knob f_form = 2 --
    // the four side by side of ru_index)
    const uint32_t sn = NW16 <= 4 ? 256u : (uint32_t)NW16 * 64u, sg = NW16 <= 4 ? 1u : 64u, lo = NW16 <= 4 ? ul * 4u : ul;
    auto ruw = [&](int n, int g) -> uint32_t { return ru[(uint32_t)n * sn + (uint32_t)g * sg + lo]; };      // (no branch around a load)
    uint32_t rn_c = ruw(wn, 0), rm_c = ruw(wm, 0);
    float4 *edge_k = reinterpret_cast<float4 *>(reinterpret_cast<char *>(ptile) + (size_t)EC * NPAIR * 128);   // [8]
    if (threadIdx.x < EC) edge_k[threadIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    {
        // Pair records from the tile's rows of lMf, every byte of the table loaded ONCE: a wave takes a group of four
        // pairs of one edge (8 patients = 384 contiguous bytes, fewer at the end of a row; missing patients read as
        // zero records), lanes 0..23 load one 16-byte value each into the wave's own LDS scratch, then every lane makes
        // the record entry of its (pair, slot) from two scratch values -- rounded ONCE to fp32.  Two groups per turn, their
        // loads in flight together.
        // (The 16 lanes of a pair loading their two operands straight from memory cost 2.9x the table's bytes in L2
        // misses at cfg5: the same line requested by several instructions in flight.)
        const int wv = (int)(threadIdx.x >> 6);
        double2 *scratch = reinterpret_cast<double2 *>(reinterpret_cast<char *>(edge_k) + 128) + wv * (2 * 24);
        fcd_f2v *dst = reinterpret_cast<fcd_f2v *>(ptile);
        const int slot = lane & 15, pl = lane >> 4;
        const int x0 = slot & 1, x1 = (slot >> 1) & 1, a0 = (slot >> 2) & 1, a1 = slot >> 3;
        const bool valid = !((x0 & a0) | (x1 & a1));
        const int l0 = a0 ? 1 : (x0 ? 2 : 0), l1 = a1 ? 1 : (x1 ? 2 : 0);          // 0 typical, 1 both, 2 discordant
        const int NG4 = (NPAIR + 3) >> 2;
        const int groups = ne * NG4, nwv = (int)(blockDim.x >> 6);
        const int row_d2 = U * 3;                                                   // 16-byte values per edge row
        const double2 *__restrict__ src = reinterpret_cast<const double2 *>(lMf + c0 * U * 6);
        for (int g0 = wv; g0 < groups; g0 += 2 * nwv) {
            double2 v[2];
            int eq[2][2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int g = g0 + t * nwv;
                const int gc = g < groups ? g : groups - 1;
                const int e = gc / NG4, q = gc - e * NG4;
                eq[t][0] = e;
                eq[t][1] = q;
                const int i2 = q * 24 + lane;                                       // value index inside the row
                // (read once, by this workgroup only: non-temporal, so the stream does not push the r words out of L2)
                if (lane < 24 && i2 < row_d2) {
                    const double *p2 = reinterpret_cast<const double *>(src + (e * row_d2 + i2));
                    v[t] = make_double2(__builtin_nontemporal_load(p2), __builtin_nontemporal_load(p2 + 1));
                } else {
                    v[t] = make_double2(0.0, 0.0);
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (lane < 24) scratch[t * 24 + lane] = v[t];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int g = g0 + t * nwv;
                const int pr = eq[t][1] * 4 + pl;
                const double2 va = scratch[t * 24 + pl * 6 + l0], vb = scratch[t * 24 + pl * 6 + 3 + l1];
                fcd_f2v r = {0.f, 0.f};
                if (valid) {
                    r.x = (float)(va.x + vb.x);
                    r.y = (float)(va.y + vb.y);
                }
                if (g < groups && pr < NPAIR) dst[(eq[t][0] * NPAIR + pr) * 16 + slot] = r;
                // the edge's bound B_e (sum over its patients of the largest |value| of the patient's row): lanes 0..7 take one
                // patient of the group each, the edge's sum gathers in LDS (any order: it only sets how cautious the draw is)
                if (g < groups && lane < 8) {
                    float a = 0.f;
#pragma unroll
                    for (int l = 0; l < 3; ++l) {
                        const double2 q = scratch[t * 24 + lane * 3 + l];
                        a = fmaxf(a, fmaxf((float)fabs(q.x), (float)fabs(q.y)));
                    }
                    atomicAdd(&edge_k[eq[t][0]].w, a * 1.0000002f);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();                                        // the scratch is free for the next turn
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    __syncthreads();
    const double lg1 = hyper[FCD_H_LNGAMMA + 1] - hyper[FCD_H_LNGAMMA + 0];
    const double lg2 = hyper[FCD_H_LNGAMMA + 2] - hyper[FCD_H_LNGAMMA + 0];
    if ((int)threadIdx.x < ne) {
        // the edge's constants as the draw wants them: the two log-odds offsets in fp32 and the error bound of the whole
        // fp32 sum (NPAIR records + the offset + the initial zero)
        const int64_t c = c0 + threadIdx.x;
        const double c1 = lg1 + (S_B[c * 3 + 1] - S_B[c * 3 + 0]), c2 = lg2 + (S_B[c * 3 + 2] - S_B[c * 3 + 0]);
        const float cm = fmaxf((float)fabs(c1), (float)fabs(c2)) * 1.0000002f;
        const float a = edge_k[threadIdx.x].w;
        edge_k[threadIdx.x] = make_float4((float)c1, (float)c2, fcd_draw_f_eta(fcd_f32_sum_err(NPAIR + 1, a) + fcd_f32_offset_err(cm, a)), 0.f);
    }
    __syncthreads();
    if (w >= GW) return;
    if (FCD_ABL(0, 3)) return;           // ablation: staging and build only
    const uint32_t chain = chain0 + (uint32_t)w * 64u + lane;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    fcd_u4 rnd = {0, 0, 0, 0};
    const int NG = (NPAIR + 7) >> 3;     // groups of 8 pairs = 16 patients = one slot word
    const uint32_t tile_off = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)ptile;   // 256-aligned

    for (int e = 0; e < ne; ++e) {
        const int64_t c = c0 + e;
        // next edge: (n, m+1), or (n+1, 0) at the end of row n (clamped past the last edge: unused there)
        int nn = wn, nm = wm + 1;
        if (nm == nn) {
            nm = 0;
            nn = (nn + 1 < Nreg) ? nn + 1 : nn;
        }
        const uint32_t tb = __builtin_amdgcn_readfirstlane(tile_off + (uint32_t)(e * NPAIR * 128));
        fcd_f2v acc = {0.f, 0.f}, acc1 = {0.f, 0.f};    // even / odd pairs: two chains of packed adds
        for (int g = 0; g < NG; ++g) {
            // slot words of the next group (of the next edge after the last group): always loaded, from a valid place
            const bool last = g + 1 == NG;
            const int pn = last ? nn : wn, pm = last ? nm : wm, pg = last ? 0 : g + 1;
            const uint32_t rn_n = ruw(pn, pg), rm_n = ruw(pm, pg);
            const uint32_t zs = (rn_c ^ rm_c) | ((rn_c & rm_c) << 2);
            const uint32_t gb = tb + (uint32_t)(g * (8 * 128));
            if (NPAIR - 8 * g >= 8) {
                fcd_f2v v[8];
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const uint32_t sh = (p == 0) ? (zs << 3) : (zs >> (4 * p - 3));
                    uint32_t ad;
                    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(ad) : "v"(sh), "s"(0x78u), "v"(gb));
                    v[p] = *(lds_cf2v *)(uintptr_t)(ad + (uint32_t)(p * 128));
                }
#pragma unroll
                for (int p = 0; p < 8; p += 2) {
                    acc += v[p];
                    acc1 += v[p + 1];
                }
            } else {
                for (int p = 0; p < NPAIR - 8 * g; ++p) {
                    const uint32_t off = ((zs >> (4 * p)) & 15u) << 3;
                    acc += *(lds_cf2v *)(uintptr_t)(off + gb + (uint32_t)(p * 128));
                }
            }
            rn_c = rn_n;
            rm_c = rm_n;
        }
        acc += acc1;
        const float4 ek = edge_k[e];
        if (e == 0 || (c & 3) == 0) rnd = fcd_philox((uint32_t)(c >> 2), chain, sweep, FCD_KIND_F, k0, k1);
        const uint32_t xw = fcd_word(rnd, (int)(c & 3));
        bool amb = false;
        int k;
        const float bf1 = ek.x + acc.x, bf2 = ek.y + acc.y, xf = (float)xw * 2.3283064e-10f;
        if (margin > 1.f || __ballot(!fcd_draw_f_sure(bf1, bf2, xf, ek.z, &k)) != 0ull) k = fcd_draw_f_fast32(bf1, bf2, xf, ek.z, margin, &amb);
        if (__ballot(amb) != 0ull) {
            // somewhere in the wave the fp32 sums cannot decide the draw: the edge again, in fp64, for the whole wave
            bool first = true;
            double b1 = 0.0, b2 = 0.0;
            const double *row = lMf + c * U * 6;
#pragma unroll 1
            for (int g = 0; g < NG; ++g) {
                const uint32_t a_ = ruw(wn, g), b_ = ruw(wm, g);
                fcd_f_exact_group(row, U, 16 * g, min(8, NPAIR - 8 * g), (a_ ^ b_) | ((a_ & b_) << 2), first, b1, b2);
            }
            b1 = lg1 + ((S_B[c * 3 + 1] - S_B[c * 3 + 0]) + b1);
            b2 = lg2 + ((S_B[c * 3 + 2] - S_B[c * 3 + 0]) + b2);
            k = fcd_draw_f(0.0, b1, b2, fcd_u32(xw));
            const bool open = fcd_f_open(b1, b2);                       // (type 0 impossible: the absolute log-weights decide)
            if (__ballot(open) != 0ull) {
                double a[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
                for (int g = 0; g < NG; ++g) {
                    const uint32_t a_ = ruw(wn, g), b_ = ruw(wm, g);
                    fcd_f_abs_group(lM + c * U * 9, U, 16 * g, min(8, NPAIR - 8 * g), (a_ ^ b_) | ((a_ & b_) << 2), a);
                }
                const int ka = fcd_f_abs_draw(S_B + c * 3, hyper, a, fcd_u32(xw));
                if (open) k = ka;
            }
            if (lane == 0) atomicAdd(&dbg->f_repeats, 1ull);
        }
        (f_state + ((int64_t)w * C + c) * 64)[(uint32_t)lane] = (uint8_t)k;     // (scalar base + lane)
        if (fsq) {
            uint8_t *sq = fsq + (int64_t)w * Nreg * Nreg * 64;
            (sq + ((int64_t)wn * Nreg + wm) * 64)[(uint32_t)lane] = (uint8_t)k;
            (sq + ((int64_t)wm * Nreg + wn) * 64)[(uint32_t)lane] = (uint8_t)k;
        }
        wn = nn;
        wm = nm;
    }
}

// conditional log-weights of every r site given the CURRENT state (nothing updated): parity hook.
__global__ __launch_bounds__(64) void gibbs_cond_r_kernel(const double *__restrict__ lM, const double *__restrict__ hyper,
                                                          const uint8_t *__restrict__ f_state,
                                                          const uint64_t *__restrict__ r_bits, int Nreg, int U, int64_t C,
                                                          int64_t G, int mode, double *__restrict__ cond_r) {
    const int u = blockIdx.x, w = blockIdx.y, n = blockIdx.z, lane = threadIdx.x;
    const uint8_t *fw = f_state + (int64_t)w * C * 64 + lane;
    double s0 = 0.0, s1 = 0.0;
    for (int m = 0; m < Nreg; ++m) {
        if (m == n) continue;
        const int64_t c = fcd_pair_to_edge(n, m, mode);
        const int k = fw[c * 64];
        const uint32_t bit = (uint32_t)((r_bits[((int64_t)w * Nreg + m) * U + u] >> lane) & 1ull);
        const double *p = lM + (c * U + u) * 9 + k * 3;
        s0 += p[bit * 2];
        s1 += p[2 - bit];
    }
    const int64_t g = (int64_t)w * 64 + lane;
    if (g < G) {
        double *o = cond_r + ((g * Nreg + n) * U + u) * 2;
        o[0] = hyper[FCD_H_LNPI0] + s0;
        o[1] = hyper[FCD_H_LNPI1] + s1;
    }
}

// ---------------------------------------------------------------------------------------------
// (pi, gamma) M-step from pooled counts c5 = {sum r, #f=0, #f=1, #f=2, chains}: the sample version of fit.py:208-220.
// Returns what hyper[i] receives (i = FCD_H_LNGAMMA + k: ln gamma_k; FCD_H_LNPI0: ln(1 - pi); FCD_H_LNPI1: ln pi), one
// logarithm per slot so that the tally's lanes 0..4 take one each; fcd_gibbs_mstep loops over the five.  C edges and
// NU = Nreg * U sites per chain.
// ---------------------------------------------------------------------------------------------
static_assert(FCD_H_LNGAMMA == 0 && FCD_H_LNPI0 == 3 && FCD_H_LNPI1 == 4, "fcd_mstep_log: slot i is hyper[i]");
__device__ __forceinline__ double fcd_mstep_log(int i, const unsigned long long *c5, double C, double NU) {
    const double Gtot = (double)c5[4];
    double v;
    if (i < 3) {
        const double n_f = Gtot * C;
        v = fmax((double)c5[1 + i] / n_f, 0.5 / n_f);             // fit.py:220 over chains
    } else {
        const double n_r = Gtot * NU;
        const double lo = 0.5 / n_r;
        const double pi = fmin(fmax((double)c5[0] / n_r, lo), 1.0 - lo);      // fit.py:213 over chains
        v = i == 3 ? 1.0 - pi : pi;
    }
    return log(v);
}

__global__ void gibbs_mstep_kernel(const long long *__restrict__ counts, double C, double NU, double *__restrict__ hyper) {
    unsigned long long c5[5];
    for (int i = 0; i < 5; ++i) c5[i] = (unsigned long long)counts[i];
    for (int i = 0; i < 5; ++i) hyper[i] = fcd_mstep_log(i, c5, C, NU);
}

// ---------------------------------------------------------------------------------------------
// tally: pooled counts AND marginal counters in one pass over the state (f_state is read once, 16 bytes
// per lane: a wave covers the 16 chain words x 64 chains of an edge with a single load instruction) -- and the
// odds and ends that used to be launches of their own around it:
//   * the pooled counts are summed in accumulators that belong to the context (acc[0..3] + a ticket in acc[4], zero
//     between launches): the block that draws the last ticket reads the totals, writes counts_out[0..4], runs the
//     (pi, gamma) M-step when hyper != nullptr (one rank: the statistics need no exchange) and puts the accumulators
//     back to zero -- no memset launch, no one-thread M-step launch;
//   * r_U != nullptr: the per-lane slot words of the NEXT f pass (pack_ru_kernel's job) are made here from the r
//     bits this kernel reads anyway.
// Integer sums: any order gives the same totals.
// ---------------------------------------------------------------------------------------------
struct tally_args {
    const uint8_t *f_state;
    const uint64_t *r_bits;
    int64_t C, NU, G;
    int GW, Nreg, U, NW;               // (NW slot-source words per region: pack_ru_word)
    unsigned long long *acc;           // context-owned: 4 sums + ticket
    unsigned long long *counts_out;    // nullable
    uint32_t *cnt_f, *cnt_r;           // nullable (both or neither)
    double *hyper;                     // nullable: M-step target
    uint32_t *r_U;                     // nullable: slot words of the next f pass
    uint2 *r_S;                        // nullable (with r_U; knob r_keep_words): the r words of the next blocked r pass (pack_r_item)
    uint32_t *marks;                   // nullable (with r_U): its marks, cleared
    int NBLK;                          // blocks of 16 regions
    int n_f_blocks;                    // blocks that read the f state (0: done elsewhere)
    int n_r_blocks;                    // blocks that count the r bits (at least; the f blocks do too); the rest make r_U (and r_S)
};

__global__ __launch_bounds__(1024, 8) void gibbs_tally_kernel(const tally_args a) {
    __shared__ unsigned long long red[16], redf[16][3];
    __shared__ int sh_last;
    const uint8_t *__restrict__ f_state = a.f_state;
    const uint64_t *__restrict__ r_bits = a.r_bits;
    uint32_t *__restrict__ cnt_f = a.cnt_f;
    uint32_t *__restrict__ cnt_r = a.cnt_r;
    const int64_t C = a.C, NU = a.NU, G = a.G;
    const int GW = a.GW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // blocks [0, nfb): the f state (nfb == 0: the r pass's packing launch has seen to it) -- and the r bits; blocks
    // [nfb, gridDim): the slot words of the next f pass (they run beside the others on CUs of their own instead of after them)
    const int nfb = a.n_f_blocks;
    const bool f_role = (int)blockIdx.x < nfb;
    if (f_role) {
        fcd_tally_f tf;
        tf.f_state = f_state; tf.C = C; tf.G = G; tf.GW = GW; tf.acc = a.acc; tf.cnt_f = cnt_f;
        fcd_tally_f_block<16>(tf, (int)blockIdx.x, nfb, redf);
    }
    // the r bits: every block of the first max(nfb, n_r_blocks) takes its share
    const int nrb = nfb > a.n_r_blocks ? nfb : a.n_r_blocks;
    const bool r_role = (int)blockIdx.x < nrb;
    unsigned long long cr = 0;
    for (int64_t i = r_role ? (int64_t)blockIdx.x * blockDim.x + threadIdx.x : NU; i < NU; i += (int64_t)nrb * blockDim.x) {
        uint32_t sr = 0;
        for (int w = 0; w < GW; ++w) sr += __popcll(r_bits[(int64_t)w * NU + i] & fcd_active_mask(w, G));
        if (cnt_r) atomicAdd(&cnt_r[i], sr);
        cr += sr;
    }
    if (a.r_U && (int)blockIdx.x >= nrb) {
        // slot words of the next f pass: one wave per (w, n, word) item, as pack_ru_kernel; then the next r pass's marks,
        // cleared as its packing launch would: 64 of the GW U NBLK marks per item.  Its r words are the ones the pass before
        // this launch wrote (the two buffers swap roles) -- or (r_S, knob r_keep_words) made here from the r bits, one wave
        // per (w, u, b) item that also clears the item's mark.
        const int U = a.U, NW = a.NW, NBLK = a.NBLK;
        const int n_marks = a.marks ? GW * U * NBLK : 0;
        const int items_u = GW * a.Nreg * NW, items = items_u + (a.r_S ? n_marks : (n_marks + 63) / 64);
        for (int item = ((int)blockIdx.x - nrb) * 16 + wave; item < items; item += ((int)gridDim.x - nrb) * 16) {
            if (item < items_u) {
                const int jw = item % NW, wn = item / NW;                   // wn = w*Nreg + n
                a.r_U[ru_index(wn, NW, jw, lane)] = pack_ru_word(r_bits, wn, U, jw, lane);
            } else if (!a.r_S) {
                const int m = (item - items_u) * 64 + lane;
                if (m < n_marks) a.marks[m] = 0u;
            } else {
                const int it = item - items_u, b = it % NBLK, wu = it / NBLK;      // wu = w*U + u
                if (lane == 0) a.marks[it] = 0u;
                a.r_S[(int64_t)it * 64 + lane] = fcd_r_pair_bytes(r_bits, a.Nreg, U, wu / U, wu % U, b, lane);
            }
        }
    }
    if (!a.acc) return;
    // Only the blocks that count take a ticket: the sums, the ticket and the M-step -- a chain of four trips to the memory
    // side -- then run BESIDE the blocks that make the slot words instead of behind the last of them.
    if (!r_role) return;
    // the r count: one atomic per BLOCK (same-address atomics serialise): wave sums -> LDS -> thread 0
    for (int o = 32; o > 0; o >>= 1) cr += __shfl_xor(cr, o, 64);
    if (lane == 0) red[wave] = cr;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int q = 0; q < 16; ++q) t += red[q];
        if (t) {
            // with the old value asked for, the add has been performed at the memory side once it returns: the
            // barrier below then orders it before this block's ticket (every access to acc[] is a device-scope atomic)
            const unsigned long long old = atomicAdd(&a.acc[0], t);
            asm volatile("" ::"v"(old));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) sh_last = (atomicAdd(&a.acc[4], 1ull) == (unsigned long long)nrb - 1ull) ? 1 : 0;
    __syncthreads();
    if (sh_last && threadIdx.x < 64) {
        // the five words are fetched (and reset) by five lanes at once: one memory round trip, not five in a row
        unsigned long long mine = 0;
        if (threadIdx.x < 5) mine = atomicExch(&a.acc[threadIdx.x], 0ull);     // read at the memory side and reset
        unsigned long long c5[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) c5[i] = __shfl(mine, i, 64);
        c5[4] = (unsigned long long)G;
        if (a.counts_out && threadIdx.x < 8) a.counts_out[threadIdx.x] = threadIdx.x < 5 ? c5[threadIdx.x] : 0ull;
        if (a.hyper && threadIdx.x < 5)      // the M-step, one logarithm per lane
            a.hyper[threadIdx.x] = fcd_mstep_log((int)threadIdx.x, c5, (double)C, (double)NU);
    }
}

// ---------------------------------------------------------------------------------------------
// log-joint per chain: grid = (GW, LJ_SLICES); slice s sums edges c = s, s+LJ_SLICES, ... and (slice 0) the
// prior of r; partial[s][g] in the workspace, folded in slice order.
// ---------------------------------------------------------------------------------------------
constexpr int LJ_SLICES = 64;
__global__ __launch_bounds__(64) void gibbs_logjoint_kernel(const double *__restrict__ S_B, const double *__restrict__ lM,
                                                            const double *__restrict__ hyper,
                                                            const uint8_t *__restrict__ f_state,
                                                            const uint64_t *__restrict__ r_bits, int Nreg, int U, int64_t C,
                                                            int GW, double *__restrict__ partial) {
    const int w = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    const uint64_t *rw = r_bits + (int64_t)w * Nreg * U;
    double acc = 0.0;
    for (int64_t c = s; c < C; c += LJ_SLICES) {
        int n, m;
        fcd_edge_to_pair(c, n, m);
        const int k = f_state[((int64_t)w * C + c) * 64 + lane];
        double e = hyper[FCD_H_LNGAMMA + k] + S_B[c * 3 + k];
        for (int u = 0; u < U; ++u) {
            const uint32_t a = (uint32_t)((rw[(int64_t)n * U + u] >> lane) & 1ull);
            const uint32_t b2 = (uint32_t)((rw[(int64_t)m * U + u] >> lane) & 1ull);
            const int l = (a & b2) ? 1 : ((a ^ b2) ? 2 : 0);
            e += lM[(c * U + u) * 9 + k * 3 + l];
        }
        acc += e;
    }
    if (s == 0) {
        int ones = 0;
        for (int64_t i = 0; i < (int64_t)Nreg * U; ++i) ones += (int)((rw[i] >> lane) & 1ull);
        acc += (double)ones * hyper[FCD_H_LNPI1] + (double)((int64_t)Nreg * U - ones) * hyper[FCD_H_LNPI0];
    }
    partial[((int64_t)s * GW + w) * 64 + lane] = acc;
}

// per-chain number of anomalous (region, patient) sites: sum_{n,u} r_nu -- the scalar SURVEY.md section 8f item 4 names
// for the chain diagnostics next to the log-joint.  One wave per (chain word, slice of the sites); out is zeroed first.
__global__ __launch_bounds__(64) void gibbs_rsum_kernel(const uint64_t *__restrict__ r_bits, int64_t NU, int64_t G,
                                                        unsigned int *__restrict__ out) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const uint64_t *rw = r_bits + (int64_t)w * NU;
    unsigned int ones = 0;
    for (int64_t i = blockIdx.y; i < NU; i += gridDim.y) ones += (unsigned int)((rw[i] >> lane) & 1ull);
    const int64_t g = (int64_t)w * 64 + lane;
    if (g < G && ones) atomicAdd(&out[g], ones);
}

__global__ void gibbs_logjoint_fold(const double *__restrict__ partial, int64_t GWx64, int64_t G, double *__restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double acc = 0.0;
    for (int s = 0; s < LJ_SLICES; ++s) acc += partial[(int64_t)s * GWx64 + g];
    out[g] = acc;
}

// ---------------------------------------------------------------------------------------------
// packed <-> plain state
// ---------------------------------------------------------------------------------------------
__global__ void export_f_kernel(const uint8_t *__restrict__ f_state, int64_t C, int64_t G, uint8_t *__restrict__ f) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over G*C, c fastest
    if (i >= G * C) return;
    const int64_t g = i / C, c = i % C;
    f[i] = f_state[((g >> 6) * C + c) * 64 + (g & 63)];
}
__global__ void export_r_kernel(const uint64_t *__restrict__ r_bits, int64_t NU, int64_t G, uint8_t *__restrict__ r) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over G*NU
    if (i >= G * NU) return;
    const int64_t g = i / NU, j = i % NU;
    r[i] = (uint8_t)((r_bits[(g >> 6) * NU + j] >> (g & 63)) & 1ull);
}
__global__ void import_f_kernel(const uint8_t *__restrict__ f, int64_t C, int64_t G, int GW, uint8_t *__restrict__ f_state) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over GW*C*64
    if (i >= (int64_t)GW * C * 64) return;
    const int64_t lane = i & 63, c = (i >> 6) % C, w = (i >> 6) / C;
    const int64_t g = w * 64 + lane;
    f_state[i] = g < G ? f[g * C + c] : 0;
}
__global__ __launch_bounds__(256) void import_r_kernel(const uint8_t *__restrict__ r, int64_t NU, int64_t G, int GW,
                                                       uint64_t *__restrict__ r_bits) {
    const int lane = threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // over GW*NU
    if (word >= (int64_t)GW * NU) return;
    const int64_t w = word / NU, j = word % NU;
    const int64_t g = w * 64 + lane;
    const uint64_t ball = __ballot(g < G ? (r[g * NU + j] != 0) : false);
    if (lane == 0) r_bits[word] = ball;
}

__global__ void philox_uniforms_kernel(const uint32_t *__restrict__ ctr4, int64_t n, uint64_t seed, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const fcd_u4 x = fcd_philox(ctr4[i * 4 + 0], ctr4[i * 4 + 1], ctr4[i * 4 + 2], ctr4[i * 4 + 3], (uint32_t)seed,
                                (uint32_t)(seed >> 32));
    out[i * 2 + 0] = fcd_u53(x.x, x.y);
    out[i * 2 + 1] = fcd_u53(x.z, x.w);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// edges per LDS tile of the f step and waves per block
void f_step_geometry(int64_t U, int GW, int &Ec, int &wpb, size_t &shmem) {
    wpb = GW < 16 ? GW : 16;
    const size_t per_edge = (size_t)U * 72;
    int64_t e = (int64_t)(32 * 1024 / per_edge);
    if (e < 1) e = 1;
    if (e > 8) e = 8;
    if (e > 1) e &= ~1ll;  // even: both halves of a Philox block are used inside one tile
    Ec = (int)e;
    shmem = per_edge * Ec;
}

template <bool COND>
int launch_f(fcd_ctx *ctx, const double *S_B, const double *lM, const double *hyper, uint8_t *f_state,
             const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, const fcd_geo &g, int64_t chain0, uint64_t seed,
             int64_t sweep, double *cond_f, hipStream_t s) {
    int Ec, wpb;
    size_t shmem;
    f_step_geometry(U, g.GW, Ec, wpb, shmem);
    if (shmem > 160 * 1024)
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "f step: one edge's table row (U=%lld patients) exceeds the 160 KiB LDS", U);
    {
        int rc = fcd_lds_attr(ctx, COND ? FCD_KA_F_COND : FCD_KA_F_GENERIC, reinterpret_cast<const void *>(&gibbs_f_kernel<COND>), shmem);
        if (rc) return rc;
    }
    dim3 grid((unsigned)((g.C + Ec - 1) / Ec), (unsigned)((g.GW + wpb - 1) / wpb));
    hipLaunchKernelGGL(gibbs_f_kernel<COND>, grid, dim3(64 * wpb), shmem, s, S_B, lM, hyper, f_state, r_bits, (int)Nreg,
                       (int)U, g.C, g.GW, G, Ec, (uint32_t)chain0, seed, (uint32_t)sweep, cond_f);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

}  // namespace

extern "C" int fcd_gibbs_state_size(int64_t Nreg, int64_t U, int64_t G, size_t *f_bytes, size_t *r_bytes) {
    if (Nreg < 2 || U < 1 || G < 1 || !f_bytes || !r_bytes) return FCD_ERR_ARG;
    const int64_t GW = (G + 63) / 64;
    *f_bytes = (size_t)(GW * fcd_tri(Nreg) * 64);
    *r_bytes = (size_t)(GW * Nreg * U * 8);
    return FCD_OK;
}

extern "C" int fcd_gibbs_init(fcd_ctx *ctx, uint8_t *f_state, uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                              int64_t chain0, uint64_t seed, double pi, fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, chain0, g);
    if (rc) return rc;
    if (!f_state || !r_bits) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_init: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t items_f = (g.C + 1) / 2 * g.GW;
    hipLaunchKernelGGL(gibbs_init_f, dim3((unsigned)((items_f + 3) / 4)), dim3(256), 0, s, f_state, g.C, g.GW,
                       (uint32_t)chain0, seed);
    FCD_LAUNCH_CHECK();
    const int64_t items_r = (Nreg + 1) / 2 * U * g.GW;
    hipLaunchKernelGGL(gibbs_init_r, dim3((unsigned)((items_r + 3) / 4)), dim3(256), 0, s, r_bits, (int)Nreg, (int)U, g.GW,
                       (uint32_t)chain0, seed, pi);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_gibbs_edge_tables(fcd_ctx *ctx, const double *lM, int64_t Nreg, int64_t U, double *lMf,
                                     fcd_stream stream) {
    if (!ctx || !lM || !lMf) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_edge_tables: null pointer");
    if (Nreg < 2 || U < 1) return fcd_fail(ctx, FCD_ERR_SHAPE, "need Nreg >= 2 and U >= 1 (Nreg=%lld, U=%lld)", Nreg, U);
    const int64_t n_items = fcd_tri(Nreg) * U;
    int64_t blocks = (n_items + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cu * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(edge_tables_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, lM, n_items, lMf);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

int fcd_sweep_call_check(fcd_ctx *ctx, fcd_sweep_call &c, bool f_pass, bool r_pass, const char *who) {
    int rc = fcd_geo_check(ctx, c.Nreg, c.U, c.G, c.chain0, c.g);
    if (rc) return rc;
    const bool null = (f_pass && !c.S_B) || !c.lM || !c.hyper || !c.f_state || !c.r_bits;
    if (null || (r_pass && c.edge_mode != FCD_EDGE_REFERENCE && c.edge_mode != FCD_EDGE_SYMMETRIC)) {
        snprintf(ctx->msg, sizeof(ctx->msg), null ? "%s: null pointer" : "%s: bad edge_mode", who);
        return FCD_ERR_ARG;
    }
    // the passes read and write 16 bytes of an f_state line per lane and take the difference tables as double2
    FCD_ALIGN16(ctx, who, "f_state", c.f_state);
    FCD_ALIGN16(ctx, who, "lMf", c.lMf);
    FCD_ALIGN16(ctx, who, "lMd", c.lMd);
    if (r_pass && c.edge_mode == FCD_EDGE_REFERENCE && c.Nreg == 2)
        return fcd_fail(ctx, FCD_ERR_INDEX, "reference edge ids: index 1 is out of bounds for axis 0 with size 1 (Nreg=2)");
    c.pl = fcd_sweep_plan_for(ctx, c.Nreg, c.U, c.g.GW);
    return FCD_OK;
}

extern "C" int fcd_gibbs_f_step(fcd_ctx *ctx, const double *S_B, const double *lM, const double *lMf, const double *hyper,
                                uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                                int64_t chain0, uint64_t seed, int64_t sweep, fcd_stream stream) {
    fcd_sweep_call c = {S_B, lM, lMf, nullptr, hyper, f_state, const_cast<uint64_t *>(r_bits) /* (read only) */, Nreg, U, G,
                        chain0, seed, FCD_EDGE_SYMMETRIC, (hipStream_t)stream};
    int rc = fcd_sweep_call_check(ctx, c, true, false, "fcd_gibbs_f_step");
    fcd_sweep_step st = {sweep};
    return rc ? rc : fcd_gibbs_f_pass(ctx, c, st);
}

int fcd_gibbs_f_pass(fcd_ctx *ctx, const fcd_sweep_call &c, fcd_sweep_step &st) {
    const fcd_sweep_plan &pl = c.pl;
    const fcd_geo &g = c.g;
    const int64_t Nreg = c.Nreg, U = c.U;
    hipStream_t s = c.s;
    const int form = c.lMf ? pl.f_form : FCD_F_GENERIC;
    if (form == FCD_F_GENERIC)
        return launch_f<false>(ctx, c.S_B, c.lM, c.hyper, c.f_state, c.r_bits, Nreg, U, c.G, g, c.chain0, c.seed, st.sweep,
                               nullptr, s);
    fcd_abl_refresh(s);
    const int wpb = g.GW < 16 ? g.GW : 16;
    float margin = FCD_DRAW_F_MARGIN;
    if ((float)ctx->knobs.f_tol > margin) margin = (float)ctx->knobs.f_tol;   // test hook: huge = every draw through fcd_draw_f
    int rc;
    if (form == FCD_F_PAIR || form == FCD_F_PAIRX) {
        // pair / triple forms: per-lane slot words over patients (scratch in the ctx workspace), records in LDS
        rc = fcd_ws_reserve(ctx, pl.ws_bytes);
        if (rc) return rc;
        uint32_t *r_U = (uint32_t *)((char *)ctx->ws.p + pl.r_U);
        if (!st.ru_ready) {     // (inside the sweep loop the previous sweep's tally has made them already)
            const int64_t items = (int64_t)g.GW * Nreg * pl.f_NW;
            hipLaunchKernelGGL(pack_ru_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, c.r_bits, (int)Nreg, (int)U,
                               pl.f_NW, g.GW, r_U);
            FCD_LAUNCH_CHECK();
        }
        dim3 grid((unsigned)((g.C + pl.f_EC - 1) / pl.f_EC), (unsigned)((g.GW + wpb - 1) / wpb));
        // pair-aligned tiles that write the r pass's f words themselves (fcd_sweep_step::f_packed; U <= 64 kernel only)
        const bool pt = st.f_packed && form == FCD_F_PAIR;
        if (st.f_rec && (!pt || !pl.frec_bytes || ctx->frec.bytes < pl.frec_bytes))
            return fcd_fail(ctx, FCD_ERR_ARG, "f pass: prebuilt records asked for where the plan has none");
        const size_t f_shmem = st.f_rec ? pl.f_shmem_rec : pl.f_shmem;
        if (st.f_packed && (form != FCD_F_PAIR || !pl.r_blocked || st.fsq))
            return fcd_fail(ctx, FCD_ERR_ARG, "f pass: packed f words asked for where the plan has none");
        uint2 *f_S = pt ? (uint2 *)((char *)ctx->ws.p + pl.f_S) : nullptr;
        const int NBLK = (int)((Nreg + R_NB - 1) / R_NB);
        if (pt) grid.x = (unsigned)fpt_tiles((Nreg + 1) / 2);
#define FCD_F_ARGS c.S_B, c.lMf, c.hyper, c.f_state, r_U, (int)Nreg, (int)U, g.C, g.GW, (uint32_t)c.chain0, c.seed, (uint32_t)st.sweep, margin, st.fsq
#define FCD_LAUNCH_F(KERN, SLOT, EXTRA)                                                                            \
    do {                                                                                                      \
        rc = fcd_lds_attr(ctx, SLOT, reinterpret_cast<const void *>(&KERN), f_shmem);                         \
        if (rc) return rc;                                                                                    \
        {                                                                                                     \
            static int lds0 = 0; /* (the pair form's record addresses start at LDS address 0) */              \
            rc = fcd_static_lds_check(ctx, reinterpret_cast<const void *>(&KERN), &lds0);                     \
            if (rc) return rc;                                                                                \
        }                                                                                                     \
        fcd_prof_begin(ctx, FCD_PROF_F, s);                                                                   \
        hipLaunchKernelGGL(KERN, grid, dim3(64 * wpb), f_shmem, s, FCD_F_ARGS, EXTRA);                        \
        fcd_prof_end(ctx, FCD_PROF_F, s);                                                                     \
    } while (0)
#define FCD_PX ctx->words, c.lM
#define FCD_PT f_S, NBLK, ctx->words, (const char *)st.f_rec, c.lM
        const bool sure = form == FCD_F_PAIR && pt && st.f_rec && st.f_sure && !(margin > 1.f) && ctx->knobs.f_sure != 1;
        if (sure && ctx->knobs.f_runs != 1 && (st.f_all || ctx->knobs.f_runs == 2)) {
            // every tile decided at the hint (or knob f_runs = 2): the decided path in block-wide runs -- no dynamic LDS
            const int rw = wpb < FR_WAVES ? wpb : FR_WAVES;
            dim3 rgrid((unsigned)fpr_runs((Nreg + 1) / 2), (unsigned)((g.GW + rw - 1) / rw));
            // The f half of the sweep's tally rides in this launch (the kernel counts what it stores) where nothing else
            // carries it for less: ahead of a sparse r pass, which has no packing launch and no waiting workgroups.  Knob
            // tally_in_f: 1 = never, 2 = wherever this form runs.
            const fcd_tally_f *tf = nullptr;
            if (st.tally_f && !st.tally_f_done && ctx->knobs.tally_in_f != 1 && (st.r_sure || ctx->knobs.tally_in_f == 2))
                tf = st.tally_f;
            fcd_prof_begin(ctx, FCD_PROF_F, s);
            hipLaunchKernelGGL(gibbs_f_run_kernel, rgrid, dim3(64 * rw), 0, s, c.S_B, c.lMf, c.hyper, c.f_state, r_U, (int)Nreg, (int)U, g.C,
                               g.GW, (uint32_t)c.chain0, c.seed, (uint32_t)st.sweep, margin, f_S, NBLK, ctx->words,
                               (const char *)st.f_rec, c.lM, (int)grid.x, (unsigned *)((char *)st.f_rec + pl.frec_votes), c.G,
                               (tf && tf->acc) ? (unsigned long long *)ctx->f_slots : nullptr, tf ? tf->cnt_f : nullptr);
            fcd_prof_end(ctx, FCD_PROF_F, s);
            FCD_LAUNCH_CHECK();
            if (tf) {           // (only now: the launch is in the stream)
                st.tally_f_done = true;
                st.f_fold = tf->acc != nullptr;     // (the r pass folds the pooled counts into acc: fcd_f_slots_fold)
                ctx->n_f_tally += 1;
            }
            ctx->n_frec_pass += 1;
            ctx->n_fsure_pass += 1;
            ctx->n_frun_pass += 1;
        } else if (sure) {
            // (a table without decided tiles, the test hook f_tol and knob f_sure = 1 keep the kernel below)
            if (pl.f_NW == 1) FCD_LAUNCH_F((gibbs_f_pair_kernel<1, true, true, true>), FCD_KA_F_PAIR_S + 0, FCD_PT);
            else if (pl.f_NW == 2) FCD_LAUNCH_F((gibbs_f_pair_kernel<2, true, true, true>), FCD_KA_F_PAIR_S + 1, FCD_PT);
            else if (pl.f_NW == 3) FCD_LAUNCH_F((gibbs_f_pair_kernel<3, true, true, true>), FCD_KA_F_PAIR_S + 2, FCD_PT);
            else FCD_LAUNCH_F((gibbs_f_pair_kernel<4, true, true, true>), FCD_KA_F_PAIR_S + 3, FCD_PT);
            ctx->n_frec_pass += 1;
            ctx->n_fsure_pass += 1;
        } else if (form == FCD_F_PAIR && pt && st.f_rec) {
            if (pl.f_NW == 1) FCD_LAUNCH_F((gibbs_f_pair_kernel<1, true, true>), FCD_KA_F_PAIR_R + 0, FCD_PT);
            else if (pl.f_NW == 2) FCD_LAUNCH_F((gibbs_f_pair_kernel<2, true, true>), FCD_KA_F_PAIR_R + 1, FCD_PT);
            else if (pl.f_NW == 3) FCD_LAUNCH_F((gibbs_f_pair_kernel<3, true, true>), FCD_KA_F_PAIR_R + 2, FCD_PT);
            else FCD_LAUNCH_F((gibbs_f_pair_kernel<4, true, true>), FCD_KA_F_PAIR_R + 3, FCD_PT);
            ctx->n_frec_pass += 1;
        } else if (form == FCD_F_PAIR && pt) {
            if (pl.f_NW == 1) FCD_LAUNCH_F((gibbs_f_pair_kernel<1, true>), FCD_KA_F_PAIR_T + 0, FCD_PT);
            else if (pl.f_NW == 2) FCD_LAUNCH_F((gibbs_f_pair_kernel<2, true>), FCD_KA_F_PAIR_T + 1, FCD_PT);
            else if (pl.f_NW == 3) FCD_LAUNCH_F((gibbs_f_pair_kernel<3, true>), FCD_KA_F_PAIR_T + 2, FCD_PT);
            else FCD_LAUNCH_F((gibbs_f_pair_kernel<4, true>), FCD_KA_F_PAIR_T + 3, FCD_PT);
        } else if (form == FCD_F_PAIR) {
            if (pl.f_NW == 1) FCD_LAUNCH_F((gibbs_f_pair_kernel<1, false>), FCD_KA_F_PAIR + 0, FCD_PT);
            else if (pl.f_NW == 2) FCD_LAUNCH_F((gibbs_f_pair_kernel<2, false>), FCD_KA_F_PAIR + 1, FCD_PT);
            else if (pl.f_NW == 3) FCD_LAUNCH_F((gibbs_f_pair_kernel<3, false>), FCD_KA_F_PAIR + 2, FCD_PT);
            else FCD_LAUNCH_F((gibbs_f_pair_kernel<4, false>), FCD_KA_F_PAIR + 3, FCD_PT);
        } else {
            if (pl.f_EC == 8) FCD_LAUNCH_F(gibbs_f_pairx_kernel<8>, FCD_KA_F_PAIR_BIG + 0, FCD_PX);
            else if (pl.f_EC == 4) FCD_LAUNCH_F(gibbs_f_pairx_kernel<4>, FCD_KA_F_PAIR_BIG + 1, FCD_PX);
            else if (pl.f_EC == 2) FCD_LAUNCH_F(gibbs_f_pairx_kernel<2>, FCD_KA_F_PAIR_BIG + 2, FCD_PX);
            else FCD_LAUNCH_F(gibbs_f_pairx_kernel<1>, FCD_KA_F_PAIR_BIG + 3, FCD_PX);
        }
#undef FCD_PT
#undef FCD_PX
#undef FCD_LAUNCH_F
#undef FCD_F_ARGS
        FCD_LAUNCH_CHECK();
        return FCD_OK;
    }
    // a patient row that fits no pair tile (U > 1280): log-odds form with scalar r masks
    rc = fcd_lds_attr(ctx, FCD_KA_F_DIFF, reinterpret_cast<const void *>(&gibbs_f_diff_kernel), pl.f_shmem);
    if (rc) return rc;
    dim3 grid((unsigned)((g.C + pl.f_EC - 1) / pl.f_EC), (unsigned)((g.GW + wpb - 1) / wpb));
    fcd_prof_begin(ctx, FCD_PROF_F, s);
    hipLaunchKernelGGL(gibbs_f_diff_kernel, grid, dim3(64 * wpb), pl.f_shmem, s, c.S_B, c.lMf, c.hyper, c.f_state, c.r_bits,
                       (int)Nreg, (int)U, g.C, g.GW, pl.f_EC, (uint32_t)c.chain0, c.seed, (uint32_t)st.sweep, margin, c.lM);
    fcd_prof_end(ctx, FCD_PROF_F, s);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_gibbs_mstep(fcd_ctx *ctx, const int64_t *counts, int64_t Nreg, int64_t U, double *hyper,
                               fcd_stream stream) {
    if (!ctx || !counts || !hyper) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_mstep: null pointer");
    if (Nreg < 2 || U < 1) return fcd_fail(ctx, FCD_ERR_SHAPE, "need Nreg >= 2 and U >= 1 (Nreg=%lld, U=%lld)", Nreg, U);
    hipLaunchKernelGGL(gibbs_mstep_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long *>(counts), (double)fcd_tri(Nreg), (double)(Nreg * U), hyper);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

// one launch of gibbs_tally_kernel; counts / cnt_f+cnt_r / hyper / r_U each optional
static int launch_tally(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                        const fcd_geo &g, int64_t *counts, uint32_t *cnt_f, uint32_t *cnt_r, double *hyper, uint32_t *r_U,
                        int ru_words, hipStream_t s, bool f_done = false, uint2 *r_S = nullptr, uint32_t *marks = nullptr) {
    tally_args a;
    a.f_state = f_state; a.r_bits = r_bits;
    a.C = g.C; a.NU = Nreg * U; a.G = G;
    a.GW = g.GW; a.Nreg = (int)Nreg; a.U = (int)U; a.NW = ru_words;
    a.marks = r_U ? marks : nullptr; a.r_S = a.marks ? r_S : nullptr;
    a.NBLK = (int)((Nreg + R_NB - 1) / R_NB);
    a.acc = (counts || hyper) ? (unsigned long long *)ctx->acc : nullptr;
    a.counts_out = reinterpret_cast<unsigned long long *>(counts);
    a.cnt_f = cnt_f; a.cnt_r = cnt_r;
    a.hyper = hyper; a.r_U = r_U;
    int64_t blocks = (g.C + 63) / 64;          // 16 waves x 4 edges per workgroup and round
    const int64_t cap = (int64_t)ctx->num_cu * 2;      // (8 per CU measured slower: 19.6 us against 15.6 us at cfg3)
    if (blocks > cap) blocks = cap;
    a.n_f_blocks = f_done ? 0 : (int)blocks;
    {   // the r bits alone: one thread per (region, patient), a few blocks
        int64_t rb = (a.NU + 1023) / 1024;
        if (rb > 64) rb = 64;
        a.n_r_blocks = (int)rb;
        // the kernel's counting blocks are the first max(n_f_blocks, n_r_blocks): the grid must hold every one of them
        if (rb > a.n_f_blocks) blocks = rb;
    }
    if (r_U) {
        const int64_t n_marks = a.marks ? (int64_t)g.GW * U * a.NBLK : 0;
        int64_t ru_blocks = ((int64_t)g.GW * Nreg * a.NW + (a.r_S ? n_marks : (n_marks + 63) / 64) + 15) / 16;
        // At most one per CU.  With the f half counted elsewhere the grid is then one round of the device's places (two
        // 1024-thread workgroups per CU: 10 + 256 of 512 at cfg3); filling the round -- 2 num_cu less the counting workgroups,
        // 1.6 items per wave instead of 3.2 -- measured the same (profiles/tally_in_r_pass_cfg3.txt).
        if (ru_blocks > ctx->num_cu) ru_blocks = ctx->num_cu;
        blocks += ru_blocks;
    }
    hipLaunchKernelGGL(gibbs_tally_kernel, dim3((unsigned)blocks), dim3(1024), 0, s, a);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_gibbs_tally(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U,
                               int64_t G, int64_t *counts, uint32_t *cnt_f, uint32_t *cnt_r, fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!f_state || !r_bits) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_tally: null pointer");
    FCD_ALIGN16(ctx, "fcd_gibbs_tally", "f_state", f_state);          // gibbs_tally_kernel reads 16 bytes of a line per lane
    if ((cnt_f == nullptr) != (cnt_r == nullptr)) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_tally: cnt_f and cnt_r go together");
    if (!counts && !cnt_f) return FCD_OK;
    return launch_tally(ctx, f_state, r_bits, Nreg, U, G, g, counts, cnt_f, cnt_r, nullptr, nullptr, 0, (hipStream_t)stream);
}

// pooled counts alone: the tally with no counters (counts[0..7] overwritten)
extern "C" int fcd_gibbs_stats(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U,
                               int64_t G, int64_t *counts, fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!f_state || !r_bits || !counts) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_stats: null pointer");
    FCD_ALIGN16(ctx, "fcd_gibbs_stats", "f_state", f_state);          // gibbs_tally_kernel reads 16 bytes of a line per lane
    return launch_tally(ctx, f_state, r_bits, Nreg, U, G, g, counts, nullptr, nullptr, nullptr, nullptr, 0, (hipStream_t)stream);
}

// marginal counters alone: the tally with no counts (cnt_f, cnt_r +=)
extern "C" int fcd_gibbs_accumulate(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg,
                                    int64_t U, int64_t G, uint32_t *cnt_f, uint32_t *cnt_r, fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!f_state || !r_bits || !cnt_f || !cnt_r) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_accumulate: null pointer");
    FCD_ALIGN16(ctx, "fcd_gibbs_accumulate", "f_state", f_state);          // gibbs_tally_kernel reads 16 bytes of a line per lane
    return launch_tally(ctx, f_state, r_bits, Nreg, U, G, g, nullptr, cnt_f, cnt_r, nullptr, nullptr, 0, (hipStream_t)stream);
}

// One row per slot of fcd_ctx::sweep_acc: fcd_gibbs_run's refusal of an accumulator made for another shape, and the launch
// that adds the counts of a state to its buffers.
static int acc_launch_pair(fcd_ctx *ctx, const fcd_sweep_call &c, const fcd_geo &g, const fcd_sweep_acc &a, hipStream_t s) {
    return fcd_pair_tally_launch<uint32_t>(ctx, c.f_state, c.r_bits, c.Nreg, c.U, c.G, g, a.buf[0], true, s);
}
static int acc_launch_count(fcd_ctx *ctx, const fcd_sweep_call &c, const fcd_geo &g, const fcd_sweep_acc &a, hipStream_t s) {
    return fcd_count_tally_launch(ctx, c.r_bits, c.Nreg, c.U, c.G, g, a.buf[0], a.buf[1], s);
}
static int acc_launch_coanomaly(fcd_ctx *ctx, const fcd_sweep_call &c, const fcd_geo &g, const fcd_sweep_acc &a, hipStream_t s) {
    return fcd_coanomaly_tally_launch(ctx, c.r_bits, c.Nreg, c.U, c.G, g, a.buf[0], a.buf[1], s);
}
static int acc_launch_region_set(fcd_ctx *ctx, const fcd_sweep_call &c, const fcd_geo &g, const fcd_sweep_acc &a, hipStream_t s) {
    return fcd_region_set_tally_launch(ctx, c.r_bits, c.Nreg, c.U, c.G, g, a.buf[0], a.buf[1], s);
}
static int acc_launch_patient_group(fcd_ctx *ctx, const fcd_sweep_call &c, const fcd_geo &g, const fcd_sweep_acc &a, hipStream_t s) {
    return fcd_patient_group_tally_launch(ctx, c.r_bits, c.Nreg, c.U, c.G, g, a.buf[0], a.buf[1], s);
}
static int acc_launch_patient_trait(fcd_ctx *ctx, const fcd_sweep_call &c, const fcd_geo &g, const fcd_sweep_acc &a, hipStream_t s) {
    return fcd_patient_trait_tally_launch(ctx, c.r_bits, c.Nreg, c.U, c.G, g, a.buf[0], (int64_t *)a.buf[1], s);
}
static const struct {
    const char *msg_shape;
    int (*launch)(fcd_ctx *, const fcd_sweep_call &, const fcd_geo &, const fcd_sweep_acc &, hipStream_t);
    int (*reserve)(fcd_ctx *, int64_t Nreg, int64_t U, int64_t G);     // its scratch (fcd_gibbs_run: before the loop), or nullptr
} SWEEP_ACC[FCD_ACC_N] = {
    {"fcd_gibbs_run: the attached pair accumulator was made for Nreg=%lld, U=%lld", acc_launch_pair, nullptr},
    {"fcd_gibbs_run: the attached count accumulator was made for Nreg=%lld, U=%lld", acc_launch_count, fcd_count_ws_reserve},
    {"fcd_gibbs_run: the attached co-anomaly accumulator was made for Nreg=%lld, U=%lld", acc_launch_coanomaly, nullptr},
    {"fcd_gibbs_run: the attached region-set accumulator was made for Nreg=%lld, U=%lld", acc_launch_region_set,
     fcd_region_set_ws_reserve},
    {"fcd_gibbs_run: the attached patient-group accumulator was made for Nreg=%lld, U=%lld", acc_launch_patient_group,
     fcd_patient_group_ws_reserve},
    {"fcd_gibbs_run: the attached patient-trait accumulator was made for Nreg=%lld, U=%lld", acc_launch_patient_trait,
     fcd_patient_trait_ws_reserve},
};

// The sampler loop of ONE rank between two exchanges of pooled statistics: fcd_gibbs_run (what UnsharedRegionFit(method=
// 'gibbs'), run_chains and bench.py call) and fcd_gibbs_sweeps.  Per sweep: f pass (1 launch), packing for the r pass (1, in
// the first sweep of a call only where the f pass can write the packed f words: packed_ok), r pass (one pipelined launch, or
// ceil(Nreg/16) + 1 block steps), tally (1) -- the tally also carries the M-step, the slot words of the next f pass and, with
// packed_ok, the cleared marks of the next r pass (whose r words are the ones this pass wrote); its f half rides in the packing
// launch or in the pipelined r pass where they take it.  hyper_m: what the M-step writes (nullptr when mstep_every == 0); acc_mask: the
// slots of the context's sweep accumulators to add to (bit k = slot k).
// The hint of a build just queued (gibbs_f_hint_kernel writes 4 build + 2 all + any, gibbs_r_hint_kernel 4 build + 2 any + share):
// polled in its pinned word (ctx->hint->f or ->r) for as long as a build can reasonably take, then behind a synchronisation of
// the stream.  n_build: the number of the build awaited; msg: what to say where none arrives; bit0 / bit1: the hint's two low
// bits.  The r pass's bound build runs behind the call's first sweep, so its wait lasts until the device has finished that
// sweep -- once per call, with the second sweep already queued.
static int fcd_hint_wait(fcd_ctx *ctx, hipStream_t s, const volatile unsigned *word, long long n_build, const char *msg, bool &bit0,
                         bool &bit1) {
    const unsigned build = (unsigned)(n_build & 0x3fffffff);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned v = *word;
    for (unsigned spin = 1; (v >> 2) != build; ++spin, v = *word) {
        if ((spin & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            FCD_HIP_TRY(hipStreamSynchronize(s));
            v = *word;
            if ((v >> 2) != build) return fcd_fail(ctx, FCD_ERR_DEVICE, msg);
            break;
        }
    }
    bit0 = (v & 1u) != 0u;
    bit1 = (v & 2u) != 0u;
    return FCD_OK;
}

static int sweep_loop(fcd_ctx *ctx, const fcd_sweep_call &c, int64_t sweep0, int64_t n_sweeps, int64_t mstep_every,
                      int64_t accumulate_from, int64_t *counts, uint32_t *cnt_f, uint32_t *cnt_r, double *hyper_m,
                      unsigned acc_mask) {
    if (n_sweeps < 0 || sweep0 < 0 || sweep0 + n_sweeps > (1ll << 32))
        return fcd_fail(ctx, FCD_ERR_ARG, "sweep range [%lld, +%lld) outside the 32-bit counter word", sweep0, n_sweeps);
    const fcd_sweep_plan &pl = c.pl;
    const fcd_geo &g = c.g;
    const int64_t Nreg = c.Nreg, U = c.U, G = c.G;
    hipStream_t s = c.s;
    const bool pair_form = c.lMf && (pl.f_form == FCD_F_PAIR || pl.f_form == FCD_F_PAIRX);
    fcd_sweep_step st = {sweep0};
    // the square copy of the f state: where the plan has one, both tables are there and the edge ids are symmetric
    uint8_t *fsq = nullptr;
    if (pl.fsq_bytes && c.lMf && c.lMd && c.edge_mode == FCD_EDGE_SYMMETRIC) {
        int rc = fcd_buf_reserve(ctx, ctx->fsq, pl.fsq_bytes);
        if (rc) return rc;
        fsq = (uint8_t *)ctx->fsq.p;
    }
    // From the second sweep of a call on, the U <= 64 f pass writes the r pass's f words itself (pair-aligned tiles), the r
    // pass before it has left the r words and the tally before it has cleared the marks: no packing launch.  The first sweep, the any-U f kernel,
    // the reference edge ids, knob r_refill and knob f_pack = 1 keep the packing launch (from the square copy).
    const bool packed_ok = pl.f_form == FCD_F_PAIR && c.lMf && c.lMd && pl.r_blocked && pl.r_idx32 &&
                           c.edge_mode == FCD_EDGE_SYMMETRIC && ctx->knobs.f_pack != 1 && !ctx->knobs.r_refill;
    // The slot words of the f pass live behind the r pass's scratch (fcd_sweep_plan): the r pass's two buffers of panel
    // values then survive from one sweep to the next, and since a completed pipelined pass leaves every slot holding its
    // sentinel again, only the first sweep of a call has to write them (13 MB at cfg3).
    if (pair_form) {
        int rc = fcd_ws_reserve(ctx, pl.ws_bytes);      // the tally writes the next pass's slot words there
        if (rc) return rc;
    }
    // Every sweep after the first runs the pair-tile f pass where packed_ok.  A call with enough of them makes the tiles'
    // records once, before the first: the table is good for THIS call's lMf and S_B only, and no later call reads it.
    // Without the buffer (above F_REC_CAP, or no room on the device) the tiles build their own records as before.
    const int64_t pt_sweeps = packed_ok ? n_sweeps - 1 : 0;
    bool use_rec = pl.frec_bytes && ctx->knobs.f_records != 1 && pt_sweeps >= (ctx->knobs.f_records == 2 ? 1 : F_REC_MIN_SWEEPS);
    if (use_rec && fcd_buf_reserve(ctx, ctx->frec, pl.frec_bytes) != FCD_OK) {
        (void)hipGetLastError();
        use_rec = false;
    }
    // The build is queued BEFORE the first sweep (which does not read it): by the time the second sweep is queued its hint --
    // has the table decided tiles? -- has long arrived in its pinned word, and the host reads it there without a call into the
    // runtime and without the device ever running dry (fcd_hint_wait).
    bool rec_built = false;
    if (use_rec) {
        ctx->n_frec_build += 1;
        hipLaunchKernelGGL(gibbs_f_records_kernel, dim3((unsigned)fpt_tiles((Nreg + 1) / 2)), dim3(64 * FP_EC), 0, s, c.S_B, c.lMf,
                           c.hyper, (int)Nreg, (int)U, (char *)ctx->frec.p, ctx->words,
                           (unsigned *)((char *)ctx->frec.p + pl.frec_votes), (int)((pl.frec_bytes - pl.frec_votes) / sizeof(unsigned)));
        FCD_LAUNCH_CHECK();
        hipLaunchKernelGGL(gibbs_f_hint_kernel, dim3(1), dim3(1), 0, s, ctx->words, &ctx->hint->f,
                           (unsigned)(ctx->n_frec_build & 0x3fffffff), c.lM, c.hyper);
        FCD_LAUNCH_CHECK();
        rec_built = true;
    }
    // The sparse r pass (fcd_gibbs_r.hip, "Decided sites of the r pass") reads bounds made once per call from the same record
    // table: where the f hint says that some tile is decided (weak tables: nothing is launched), the build is queued with the
    // sweep that learns it, its own hint -- what share of the sites is decided -- is read one sweep later, and the passes
    // from then on run the sparse form where the rule of knob r_sure chooses it.  A forced exact path (r_tol) and the knobs
    // that pick a form of the blocked pass keep the old forms.
    const fcd_knobs &kn = ctx->knobs;
    const bool rs_ok = pl.rs_bytes && kn.r_sure != 1 && !(kn.r_tol > 16.0 * FCD_LOGIT_FAST_ERR) && !kn.r_path && !kn.r_coop &&
                       !kn.r_dsplit;
    int rs_state = 0;              // 0: no build yet, 1: build queued, 2: the sparse form runs, -1: it does not
    for (int64_t i = 0; i < n_sweeps; ++i) {
        st.sweep = sweep0 + i;
        st.f_packed = packed_ok && st.r_packed;
        st.fsq = st.f_packed ? nullptr : fsq;
        if (rs_state == 1 && st.f_packed) {
            bool share = false, any = false;
            int rc = fcd_hint_wait(ctx, s, &ctx->hint->r, ctx->n_rsure_build, "r pass: the bound build left no hint", share, any);
            if (rc) return rc;
            rs_state = (kn.r_sure == 2 || share) ? 2 : -1;
        }
        if (rec_built && st.f_packed && !st.f_rec) {
            int rc = fcd_hint_wait(ctx, s, &ctx->hint->f, ctx->n_frec_build, "f pass: the record build left no hint", st.f_sure, st.f_all);
            if (rc) return rc;
            st.f_rec = ctx->frec.p;
            if (rs_ok && (st.f_sure || kn.r_sure == 2)) {
                rc = fcd_gibbs_r_bounds_build(ctx, c);
                if (rc) return rc;
                rs_state = 1;
            } else {
                rs_state = -1;
            }
        }
        st.r_sure = rs_state == 2 && st.f_packed && st.r_packed;
        const bool last = i + 1 == n_sweeps;
        const bool do_m = mstep_every > 0 && (i + 1) % mstep_every == 0;
        const bool do_a = cnt_f && st.sweep >= accumulate_from;
        // the f half of this sweep's tally rides in the f pass's run kernel, which counts what it stores, where a sparse r
        // pass follows (knob tally_in_f); else in the r pass's packing launch (beside it, not after the pass) where there
        // is one, else in the pipelined pass's in-order workgroups (while they wait) where the rule allows; else the tally
        // after the pass counts it.  Whoever carries it sets tally_f_done, and nobody behind it counts again.
        fcd_tally_f tf;
        tf.f_state = c.f_state; tf.C = g.C; tf.G = G; tf.GW = g.GW;
        tf.acc = (do_m || (last && counts)) ? (unsigned long long *)ctx->acc : nullptr;
        tf.cnt_f = do_a ? cnt_f : nullptr;
        st.tally_f = (tf.acc || tf.cnt_f) ? &tf : nullptr;
        st.tally_f_done = false;
        st.f_fold = false;
        int rc = fcd_gibbs_f_pass(ctx, c, st);
        if (rc) return rc;      // (the run kernel's launch is the pass's last step: a pass that fails has counted nothing)
        rc = fcd_gibbs_r_pass(ctx, c, st);
        if (rc) {
            // the run kernel, the packing launch or a pipelined pass may already have added this sweep's f counts into the context's accumulators and no tally
            // will draw the ticket that zeroes them: leave them clean for the next call
            if (tf.acc) (void)hipMemsetAsync(ctx->acc, 0, FCD_ACC_BYTES, s);
            // (... and a run kernel that counted has left them in its slot lines if the pass failed before it folded them)
            if (st.f_fold) (void)hipMemsetAsync(ctx->f_slots, 0, FCD_F_SLOTS_BYTES, s);
            return rc;
        }
        st.sentinels_in_place = pair_form && ctx->r_form_last == 2;        // (a pipelined pass has just been queued)
        // the r pass's scratch is dead once its last launch is queued: the slot words of the next f pass go to their place
        uint32_t *r_U_next = (pair_form && !last) ? (uint32_t *)((char *)ctx->ws.p + pl.r_U) : nullptr;
        // ... and the r words of the next r pass with its marks, cleared.  The words are there already: what this pass wrote
        // as r_Sn (the redrawn bytes of every block) is the next pass's r_S, so the two buffers swap roles -- inside this
        // call; every call starts from the plan's assignment.  Knob r_keep_words: the tally makes them from the r bits.
        const bool r_next = packed_ok && r_U_next;
        const bool keep_words = ctx->knobs.r_keep_words == 1;
        uint2 *r_S_next = (r_next && keep_words) ? (uint2 *)((char *)ctx->ws.p + (st.r_flip ? pl.r_Sn : pl.r_S)) : nullptr;
        int64_t *cts = (last ? counts : nullptr);
        // Several ranks (a communicator on the context): the tally leaves this rank's counts in the context's vector, RCCL sums
        // it over the ranks in place ON THIS STREAM, a one-thread kernel makes the M-step from the pooled counts -- all queued
        // behind one another, the host far ahead.  One rank: the M-step runs inside the tally launch.
        const bool pooled = do_m && ctx->comm != nullptr;
        int64_t *tally_counts = pooled ? (int64_t *)ctx->pool_counts : cts;
        if (do_m || do_a || cts || r_U_next) {
            rc = launch_tally(ctx, c.f_state, c.r_bits, Nreg, U, G, g, tally_counts, do_a ? cnt_f : nullptr, do_a ? cnt_r : nullptr,
                              (do_m && !pooled) ? hyper_m : nullptr, r_U_next, pl.f_NW, s, st.tally_f_done, r_S_next,
                              r_next ? (uint32_t *)((char *)ctx->ws.p + pl.marks) : nullptr);
            if (rc) {
                if (tf.acc) (void)hipMemsetAsync(ctx->acc, 0, FCD_ACC_BYTES, s);
                return rc;
            }
        }
        if (pooled) {
            rc = fcd_comm_allreduce_counts(ctx, (long long *)ctx->pool_counts, s);
            if (rc) return rc;
            hipLaunchKernelGGL(gibbs_mstep_kernel, dim3(1), dim3(1), 0, s, (const long long *)ctx->pool_counts, (double)g.C,
                               (double)(Nreg * U), hyper_m);
            FCD_LAUNCH_CHECK();
            if (cts) FCD_HIP_TRY(hipMemcpyAsync(cts, ctx->pool_counts, 8 * sizeof(long long), hipMemcpyDeviceToDevice, s));
        } else if (cts && ctx->comm) {
            // (counts asked for without an M-step in this sweep: pooled all the same -- what a caller of several ranks expects)
            rc = fcd_comm_allreduce_counts(ctx, (long long *)cts, s);
            if (rc) return rc;
        }
        // the attached accumulators' counts of the end-of-sweep state: a launch of its own each (two for the histograms)
        if (acc_mask && st.sweep >= accumulate_from) {
            for (int k = 0; k < FCD_ACC_N; ++k) {
                const fcd_sweep_acc &a = ctx->sweep_acc[k];
                if (!(acc_mask >> k & 1u) || (st.sweep - accumulate_from) % a.every != 0) continue;
                rc = SWEEP_ACC[k].launch(ctx, c, g, a, s);
                if (rc) return rc;
            }
        }
        st.ru_ready = r_U_next != nullptr;
        st.r_packed = r_next;
        if (r_next && !keep_words) st.r_flip = !st.r_flip;
    }
    return FCD_OK;
}

extern "C" int fcd_gibbs_run(fcd_ctx *ctx, const double *S_B, const double *lM, const double *lMf, const double *lMd,
                             double *hyper, uint8_t *f_state, uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                             int64_t chain0, uint64_t seed, int64_t sweep0, int64_t n_sweeps, int edge_mode,
                             int64_t mstep_every, int64_t accumulate_from, int64_t *counts, uint32_t *cnt_f, uint32_t *cnt_r,
                             fcd_stream stream) {
    fcd_sweep_call c = {S_B, lM, lMf, lMd, hyper, f_state, r_bits, Nreg, U, G, chain0, seed, edge_mode, (hipStream_t)stream};
    int rc = fcd_sweep_call_check(ctx, c, true, true, "fcd_gibbs_run");
    if (rc) return rc;
    if ((cnt_f == nullptr) != (cnt_r == nullptr)) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_run: cnt_f and cnt_r go together");
    if (mstep_every < 0) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_run: mstep_every < 0");
    unsigned acc_mask = 0;
    for (int k = 0; k < FCD_ACC_N; ++k) {
        const fcd_sweep_acc &a = ctx->sweep_acc[k];
        if (!a.buf[0]) continue;
        if (a.nreg != Nreg || a.u != U) return fcd_fail(ctx, FCD_ERR_SHAPE, SWEEP_ACC[k].msg_shape, a.nreg, a.u);
        acc_mask |= 1u << k;
    }
    for (int k = 0; k < FCD_ACC_N; ++k) {
        if (!(acc_mask >> k & 1u) || !SWEEP_ACC[k].reserve) continue;
        rc = SWEEP_ACC[k].reserve(ctx, Nreg, U, G);          // (grown here, never inside the sweep loop)
        if (rc) return rc;
    }
    return sweep_loop(ctx, c, sweep0, n_sweeps, mstep_every, accumulate_from, counts, cnt_f, cnt_r, hyper, acc_mask);
}

// fcd_gibbs_run's loop without M-step, marginal counters, pair, anomalous-region or co-anomaly counts.  The counts are made by fcd_gibbs_stats after the
// loop: this rank's own, never pooled over an attached communicator.
extern "C" int fcd_gibbs_sweeps(fcd_ctx *ctx, const double *S_B, const double *lM, const double *lMf, const double *lMd,
                                const double *hyper,
                                uint8_t *f_state, uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, int64_t chain0,
                                uint64_t seed, int64_t sweep0, int64_t n_sweeps, int edge_mode, int64_t *counts,
                                fcd_stream stream) {
    fcd_sweep_call c = {S_B, lM, lMf, lMd, hyper, f_state, r_bits, Nreg, U, G, chain0, seed, edge_mode, (hipStream_t)stream};
    int rc = fcd_sweep_call_check(ctx, c, true, true, "fcd_gibbs_sweeps");
    if (rc) return rc;
    rc = sweep_loop(ctx, c, sweep0, n_sweeps, 0, 0, nullptr, nullptr, nullptr, nullptr, 0u);
    if (rc) return rc;
    if (counts && n_sweeps > 0) return fcd_gibbs_stats(ctx, f_state, r_bits, Nreg, U, G, counts, stream);
    return FCD_OK;
}

extern "C" int fcd_gibbs_logjoint(fcd_ctx *ctx, const double *S_B, const double *lM, const double *hyper,
                                  const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                                  double *out, fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!S_B || !lM || !hyper || !f_state || !r_bits || !out) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_logjoint: null pointer");
    const size_t need = (size_t)LJ_SLICES * g.GW * 64 * sizeof(double);
    rc = fcd_ws_reserve(ctx, need);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gibbs_logjoint_kernel, dim3((unsigned)g.GW, LJ_SLICES), dim3(64), 0, s, S_B, lM, hyper, f_state,
                       r_bits, (int)Nreg, (int)U, g.C, g.GW, (double *)ctx->ws.p);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(gibbs_logjoint_fold, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, (const double *)ctx->ws.p,
                       (int64_t)g.GW * 64, G, out);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_gibbs_chain_rsum(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, uint32_t *out,
                                    fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!r_bits || !out) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_chain_rsum: null pointer");
    hipStream_t s = (hipStream_t)stream;
    FCD_HIP_TRY(hipMemsetAsync(out, 0, (size_t)G * sizeof(uint32_t), s));
    const int64_t NU = Nreg * U;
    const int slices = (int)(NU < 64 ? NU : 64);
    hipLaunchKernelGGL(gibbs_rsum_kernel, dim3((unsigned)g.GW, (unsigned)slices), dim3(64), 0, s, r_bits, NU, G, out);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_gibbs_conditionals(fcd_ctx *ctx, const double *S_B, const double *lM, const double *hyper,
                                      const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg, int64_t U,
                                      int64_t G, int edge_mode, double *cond_f, double *cond_r, fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!S_B || !lM || !hyper || !f_state || !r_bits) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_conditionals: null pointer");
    if (edge_mode != FCD_EDGE_REFERENCE && edge_mode != FCD_EDGE_SYMMETRIC)
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_conditionals: edge_mode %lld", edge_mode);
    if (edge_mode == FCD_EDGE_REFERENCE && Nreg == 2 && cond_r)
        return fcd_fail(ctx, FCD_ERR_INDEX, "reference edge ids: index 1 is out of bounds for axis 0 with size 1 (Nreg=2)");
    hipStream_t s = (hipStream_t)stream;
    if (cond_f) {
        rc = launch_f<true>(ctx, S_B, lM, hyper, const_cast<uint8_t *>(f_state), r_bits, Nreg, U, G, g, 0, 0, 0, cond_f, s);
        if (rc) return rc;
    }
    if (cond_r) {
        if (U > 65535 || Nreg > 65535) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_gibbs_conditionals: grid too large");
        hipLaunchKernelGGL(gibbs_cond_r_kernel, dim3((unsigned)U, (unsigned)g.GW, (unsigned)Nreg), dim3(64), 0, s, lM, hyper,
                           f_state, r_bits, (int)Nreg, (int)U, g.C, G, edge_mode, cond_r);
        FCD_LAUNCH_CHECK();
    }
    return FCD_OK;
}

extern "C" int fcd_gibbs_export_state(fcd_ctx *ctx, const uint8_t *f_state, const uint64_t *r_bits, int64_t Nreg,
                                      int64_t U, int64_t G, uint8_t *f, uint8_t *r, fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!f_state || !r_bits || !f || !r) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_export_state: null pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(export_f_kernel, dim3((unsigned)((G * g.C + 255) / 256)), dim3(256), 0, s, f_state, g.C, G, f);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(export_r_kernel, dim3((unsigned)((G * Nreg * U + 255) / 256)), dim3(256), 0, s, r_bits, Nreg * U, G, r);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_gibbs_import_state(fcd_ctx *ctx, const uint8_t *f, const uint8_t *r, int64_t Nreg, int64_t U,
                                      int64_t G, uint8_t *f_state, uint64_t *r_bits, fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!f_state || !r_bits || !f || !r) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_import_state: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t nf = (int64_t)g.GW * g.C * 64;
    hipLaunchKernelGGL(import_f_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, f, g.C, G, g.GW, f_state);
    FCD_LAUNCH_CHECK();
    const int64_t words = (int64_t)g.GW * Nreg * U;
    hipLaunchKernelGGL(import_r_kernel, dim3((unsigned)((words + 3) / 4)), dim3(256), 0, s, r, Nreg * U, G, g.GW, r_bits);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_philox_uniforms(fcd_ctx *ctx, const uint32_t *ctr4, int64_t n, uint64_t seed, double *out,
                                   fcd_stream stream) {
    if (!ctx || !ctr4 || !out || n < 0) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_philox_uniforms: bad argument");
    if (n == 0) return FCD_OK;
    hipLaunchKernelGGL(philox_uniforms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ctr4, n,
                       seed, out);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
