// Co-anomaly: which regions are anomalous together, and which patients share anomalous regions.
//
// Inside a patient the r_nu are coupled through the mixture cases of their edges, across patients through f (see
// fcd_count.hip): P(r_nu = 1, r_mu = 1) is not the product of the marginals, and only the chains' joint states hold it.
// Two second-moment matrices summarise that joint, both integer sums over chains of one state:
//   region_pairs[n, m]  += sum_w sum_u popc(r[w,n,u] & r[w,m,u] & m_w)     (Nreg, Nreg) uint32
//   patient_pairs[u, v] += sum_w sum_n popc(r[w,n,u] & r[w,n,v] & m_w)     (U, U)       uint32
// with m_w the chains of word w that exist (fcd_active_mask).  r_bits holds 64 chains per word, so each is a binary
// matrix product, X X^T with X = r as (Nreg, GW*U) words, and X^T X per word with X = r as (Nreg, U).  Kernels:
//   coanomaly_kernel      ONE launch for both matrices.  A workgroup takes a CO_T x CO_T output tile on or below the
//                         diagonal of one matrix and a share of the summed extent (chunks of CO_KC terms of one chain
//                         word); both operand tiles of a chunk are staged in LDS, masked there; a thread keeps 2 x 2
//                         outputs in registers over all its chunks: one AND, one 64-bit popcount and an add per term.
//                         The tile and its mirror image are then added to the matrix: in place where the workgroup owns
//                         the whole extent (no atomics, as count_hist_kernel), with integer atomics where the extent is
//                         split over workgroups to fill the machine (coanomaly_tally_launch decides; the sum is exact
//                         either way).
//   coanomaly_vb_kernel   the same two matrices if the sites were independent with marginals q_nu from lq_R (the mean
//                         field's law): sum_u q_nu q_mu and sum_n q_nu q_nv off the diagonals, sum_u q_nu and sum_n q_nu
//                         on them (r^2 = r).  fp64, summed in index order: results repeat bit for bit.
#include "fcd_tally.h"

namespace {

constexpr int CO_T = 32;                // outputs per tile side
constexpr int CO_THREADS = 256;         // 16 x 16 threads, 2 x 2 outputs each (rows ty, ty + 16; columns tx, tx + 16)
constexpr int CO_KC = 64;               // terms of the summed index per staged chunk
constexpr int CO_RS = CO_KC + 1;        // row stride of a row-major operand tile: odd, so that 16 rows fall on 16 bank pairs
constexpr int CO_TILE_WORDS = CO_T * CO_RS;
constexpr int CO_STAGE = CO_T * CO_KC / CO_THREADS;      // words per thread and operand tile
// Workgroups the launch aims for (per CU) when it splits the summed extent; 0 never splits: every tile is owned by one
// workgroup and added without atomics.  Measured (profiles/coanomaly_cost.json, one tally at cfg3 / at 400 x 500, 1024
// chains): 0: 277 / 875 us, 1: 44 / 901 us, 4: 14.6 / 306 us, 8: 10.9 / 289 us -- tiles alone leave most CUs idle, and a
// workgroup alone on its CU waits out every chunk's loads.  (tuning builds: make EXTRA='-DFCD_CO_WG_PER_CU=0')
#ifndef FCD_CO_WG_PER_CU
#define FCD_CO_WG_PER_CU 8
#endif

constexpr int VB_T = 16;                // coanomaly_vb_kernel: 16 x 16 outputs per workgroup, one per thread
constexpr int VB_KC = 32;

struct co_side {
    uint32_t *out;      // (L, L)
    int L;              // outputs per side: Nreg (region) or U (patient)
    int K;              // summed index per chain word: U (region) or Nreg (patient)
    int nt;             // tiles per side
    int nkc;            // chunks per chain word
    int split;          // workgroups per tile; > 1: atomics
    int blocks;         // nt (nt + 1) / 2 * split
};

// tile (ti, tj), ti >= tj, of the lower triangle in row order: t = ti (ti + 1) / 2 + tj
__device__ __forceinline__ void co_tile_of(int t, int &ti, int &tj) {
    int i = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (i * (i + 1) / 2 > t) --i;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    ti = i;
    tj = t - i * (i + 1) / 2;
}

// One operand tile of one chunk into LDS, masked: rows row0 .. row0 + CO_T of the output index, terms k0 .. k0 + CO_KC of
// the summed one; what lies outside the matrix is zero.
//   REGION   row = n, k = u: the source row (w, n, :) is contiguous in k; LDS [row][k], row stride CO_RS
//   patient  row = u, k = n: the source row (w, n, :) is contiguous in the output index; LDS [k][row], row stride CO_T
// Both read r_bits along u.
template <bool REGION>
__device__ __forceinline__ void co_stage(const uint64_t *__restrict__ rw, int U, int L, int K, int row0, int k0, uint64_t m,
                                         uint64_t *__restrict__ lds, int tid) {
    uint64_t v[CO_STAGE];
#pragma unroll
    for (int q = 0; q < CO_STAGE; ++q) {
        const int i = q * CO_THREADS + tid;
        const int row = row0 + (REGION ? i / CO_KC : i % CO_T);
        const int k = k0 + (REGION ? i % CO_KC : i / CO_T);
        const int64_t src = REGION ? (int64_t)row * U + k : (int64_t)k * U + row;
        v[q] = (row < L && k < K) ? rw[src] & m : 0ull;
    }
#pragma unroll
    for (int q = 0; q < CO_STAGE; ++q) {
        const int i = q * CO_THREADS + tid;
        lds[REGION ? (i / CO_KC) * CO_RS + i % CO_KC : i] = v[q];
    }
}

template <bool REGION>
__device__ __forceinline__ void co_tile(const uint64_t *__restrict__ r_bits, int Nreg, int U, int GW, int64_t G, const co_side &sd,
                                        int block, uint64_t *__restrict__ lds) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int ti, tj;
    co_tile_of(block / sd.split, ti, tj);
    const int part = block % sd.split;
    const bool diag = ti == tj;
    const int i0 = ti * CO_T, j0 = tj * CO_T;
    uint64_t *A = lds, *B = diag ? lds : lds + CO_TILE_WORDS;
    constexpr int RS = REGION ? CO_RS : 1, KS = REGION ? 1 : CO_T;       // LDS strides of (row, k)
    uint32_t acc[2][2] = {{0u, 0u}, {0u, 0u}};
    const int nchunks = GW * sd.nkc;
    for (int c = part; c < nchunks; c += sd.split) {
        const int w = c / sd.nkc, k0 = (c % sd.nkc) * CO_KC;
        const uint64_t *rw = r_bits + (int64_t)w * Nreg * U;
        const uint64_t m = fcd_active_mask(w, G);
        __syncthreads();                         // the previous chunk is read
        co_stage<REGION>(rw, U, sd.L, sd.K, i0, k0, m, A, tid);
        if (!diag) co_stage<REGION>(rw, U, sd.L, sd.K, j0, k0, m, B, tid);
        __syncthreads();
        const int kn = min(CO_KC, sd.K - k0);
#pragma unroll 4
        for (int k = 0; k < kn; ++k) {
            const uint64_t a0 = A[ty * RS + k * KS], a1 = A[(ty + 16) * RS + k * KS];
            const uint64_t b0 = B[tx * RS + k * KS], b1 = B[(tx + 16) * RS + k * KS];
            acc[0][0] += (uint32_t)__popcll(a0 & b0);
            acc[0][1] += (uint32_t)__popcll(a0 & b1);
            acc[1][0] += (uint32_t)__popcll(a1 & b0);
            acc[1][1] += (uint32_t)__popcll(a1 & b1);
        }
    }
    // through LDS, so that the tile and its mirror image both leave along rows of the matrix
    __syncthreads();
    uint32_t *T = reinterpret_cast<uint32_t *>(lds);         // [CO_T][CO_T + 1]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) T[(ty + 16 * a) * (CO_T + 1) + tx + 16 * b] = acc[a][b];
    __syncthreads();
    const bool atomic = sd.split > 1;
    const int L = sd.L;
    for (int i = tid; i < CO_T * CO_T; i += CO_THREADS) {
        const int rr = i / CO_T, cc = i % CO_T;
        if (i0 + rr < L && j0 + cc < L) {
            const uint32_t v = T[rr * (CO_T + 1) + cc];
            uint32_t *p = sd.out + (int64_t)(i0 + rr) * L + j0 + cc;
            if (v) {
                if (atomic) atomicAdd(p, v);
                else *p += v;
            }
        }
        if (!diag && j0 + rr < L && i0 + cc < L) {
            const uint32_t v = T[cc * (CO_T + 1) + rr];
            uint32_t *p = sd.out + (int64_t)(j0 + rr) * L + i0 + cc;
            if (v) {
                if (atomic) atomicAdd(p, v);
                else *p += v;
            }
        }
    }
}

// blocks 0 .. rg.blocks - 1: the region matrix; the rest: the patient matrix
__global__ __launch_bounds__(CO_THREADS) void coanomaly_kernel(const uint64_t *__restrict__ r_bits, int Nreg, int U, int GW, int64_t G,
                                                               co_side rg, co_side pt) {
    __shared__ uint64_t lds[2 * CO_TILE_WORDS];
    const int b = blockIdx.x;
    if (b < rg.blocks) co_tile<true>(r_bits, Nreg, U, GW, G, rg, b, lds);
    else co_tile<false>(r_bits, Nreg, U, GW, G, pt, b - rg.blocks, lds);
}

// Tile (by, bx) of the region matrix (blockIdx.z = 0) or the patient matrix (1); q_nu = P(r_nu = 1) from lq_R (tally_q: q = 0
// and q = 1 exact), made where the chunk is staged.  Every output sums its terms in index order.
__global__ __launch_bounds__(VB_T * VB_T) void coanomaly_vb_kernel(const double *__restrict__ lq_R, int Nreg, int U,
                                                                   double *__restrict__ region, double *__restrict__ patient) {
    __shared__ double qa[VB_T][VB_KC + 1], qb[VB_T][VB_KC + 1];
    const bool reg = blockIdx.z == 0;
    const int L = reg ? Nreg : U, K = reg ? U : Nreg;
    const int i0 = blockIdx.y * VB_T, j0 = blockIdx.x * VB_T;
    if (i0 >= L || j0 >= L) return;              // (the grid is made for the larger matrix)
    const int tid = threadIdx.x, tx = tid % VB_T, ty = tid / VB_T;
    double *out = reg ? region : patient;
    const int i = i0 + ty, j = j0 + tx;
    double s = 0.0;
    for (int k0 = 0; k0 < K; k0 += VB_KC) {
        __syncthreads();
        for (int e = tid; e < 2 * VB_T * VB_KC; e += VB_T * VB_T) {
            const int side = e / (VB_T * VB_KC), x = e % (VB_T * VB_KC);
            // region: k = u runs along lq_R's rows; patient: the output index u does
            const int row = reg ? x / VB_KC : x % VB_T, kk = reg ? x % VB_KC : x / VB_T;
            const int gr = (side ? j0 : i0) + row, gk = k0 + kk;
            double q0, q = 0.0;
            if (gr < L && gk < K) tally_q(lq_R, reg ? (int64_t)gr * U + gk : (int64_t)gk * U + gr, q0, q);
            (side ? qb : qa)[row][kk] = q;
        }
        __syncthreads();
        const int kn = min(VB_KC, K - k0);
        if (i == j) {
            for (int k = 0; k < kn; ++k) s += qa[ty][k];
        } else {
            for (int k = 0; k < kn; ++k) s += qa[ty][k] * qb[tx][k];
        }
    }
    if (i < L && j < L) out[(int64_t)i * L + j] = s;
}

co_side co_side_of(uint32_t *out, int64_t L, int64_t K, int GW, int64_t want_split) {
    co_side sd;
    sd.out = out;
    sd.L = (int)L;
    sd.K = (int)K;
    sd.nt = (int)((L + CO_T - 1) / CO_T);
    sd.nkc = (int)((K + CO_KC - 1) / CO_KC);
    const int64_t nchunks = (int64_t)GW * sd.nkc;
    sd.split = (int)(want_split < 1 ? 1 : (want_split > nchunks ? nchunks : want_split));
    sd.blocks = sd.nt * (sd.nt + 1) / 2 * sd.split;
    return sd;
}

}  // namespace

int fcd_coanomaly_tally_launch(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G, const fcd_geo &g,
                               uint32_t *region_pairs, uint32_t *patient_pairs, hipStream_t s) {
    // tiles of both matrices on or below their diagonals; with fewer of them than the machine has room for, the summed
    // extent of each is split over that many workgroups (atomics), else every tile is owned (none)
    const int64_t ntr = (Nreg + CO_T - 1) / CO_T, ntp = (U + CO_T - 1) / CO_T;
    const int64_t tiles = ntr * (ntr + 1) / 2 + ntp * (ntp + 1) / 2;
    const int64_t want = (int64_t)ctx->num_cu * FCD_CO_WG_PER_CU;
    const int64_t split = want / tiles;          // (rounded down: one where the tiles alone fill the machine)
    if (tiles * (split < 1 ? 1 : split) > 0x7fffffffll)
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "co-anomaly tally: Nreg=%lld U=%lld need too many workgroups", Nreg, U);
    const co_side rg = co_side_of(region_pairs, Nreg, U, g.GW, split);
    const co_side pt = co_side_of(patient_pairs, U, Nreg, g.GW, split);
    hipLaunchKernelGGL(coanomaly_kernel, dim3((unsigned)(rg.blocks + pt.blocks)), dim3(CO_THREADS), 0, s, r_bits, (int)Nreg, (int)U,
                       g.GW, G, rg, pt);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_gibbs_coanomaly_tally(fcd_ctx *ctx, const uint64_t *r_bits, int64_t Nreg, int64_t U, int64_t G,
                                         uint32_t *region_pairs, uint32_t *patient_pairs, fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!r_bits || !region_pairs || !patient_pairs) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_gibbs_coanomaly_tally: null pointer");
    return fcd_coanomaly_tally_launch(ctx, r_bits, Nreg, U, G, g, region_pairs, patient_pairs, (hipStream_t)stream);
}

extern "C" int fcd_gibbs_set_coanomaly_accumulator(fcd_ctx *ctx, uint32_t *region_pairs, uint32_t *patient_pairs, int64_t Nreg,
                                                   int64_t U, int64_t every) {
    return fcd_sweep_acc_set(ctx, FCD_ACC_COANOMALY, region_pairs, patient_pairs, Nreg, U, every,
                             "fcd_gibbs_set_coanomaly_accumulator: region_pairs and patient_pairs go together",
                             "fcd_gibbs_set_coanomaly_accumulator: Nreg=%lld U=%lld", nullptr,
                             "fcd_gibbs_set_coanomaly_accumulator: every=%lld must be >= 1");
}

extern "C" int fcd_vb_coanomaly(fcd_ctx *ctx, const double *lq_R, int64_t Nreg, int64_t U, double *region, double *patient,
                                fcd_stream stream) {
    if (!ctx) return FCD_ERR_ARG;
    if (!lq_R || !region || !patient) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_vb_coanomaly: null pointer");
    if (Nreg < 1 || U < 1) return fcd_fail(ctx, FCD_ERR_SHAPE, "fcd_vb_coanomaly: Nreg=%lld U=%lld", Nreg, U);
    const int64_t L = Nreg > U ? Nreg : U;
    const int64_t nt = (L + VB_T - 1) / VB_T;
    if (nt > 65535) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_vb_coanomaly: Nreg=%lld U=%lld", Nreg, U);
    hipLaunchKernelGGL(coanomaly_vb_kernel, dim3((unsigned)nt, (unsigned)nt, 2), dim3(VB_T * VB_T), 0, (hipStream_t)stream, lq_R,
                       (int)Nreg, (int)U, region, patient);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
