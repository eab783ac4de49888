// Model evidence by annealed importance sampling over the whole state (f, r): the two kernels a rung of the ladder adds to
// the sampler's sweep (fcdiff_amd/evidence.py).
//
//   evidence_energy_kernel / evidence_energy_fold
//       E_g = sum_c S_B[c, f_gc] + sum_{c,u} lM[c, u, f_gc, l(r_gnu, r_gmu)] of every chain (true endpoints of c: the mixture
//       case of gibbs_logjoint_kernel) and w[g] += (beta - beta_prev) E_g.  The same gathers as score_ais_kernel, which reads
//       lM once per chain word; here the table goes through LDS instead.  The (c, u) records of lM are contiguous (72 bytes
//       each), so a workgroup takes a contiguous range of ITEMS i = c U + u -- any U alike, U = 1 included -- stages it tile
//       by tile in LDS and every one of its waves walks the tile for a chain word of its own, lanes = chains:
//         - the f byte of an edge is one coalesced 64-byte load per wave, EV_EB edges' loads issued together;
//         - the r words of (n, u) and (m, u) are wave-uniform (scalar loads); the mixture case of the 64 chains comes from
//           the two words' AND and XOR as lane masks (two v_cndmask, no per-lane shift);
//         - the table value is one 8-byte LDS read at record + (3 f + l): the 64 lanes of a wave touch at most 9 different
//           doubles of ONE record, 72 contiguous bytes = 18 banks, every address of a bank the same (broadcast): no conflict.
//       S_B[c, k] is added into the three k rows of the record of (c, u = 0) while the tile is staged, so the walk has one
//       gather per item and nothing else.  A chain's partial sum of a slice is made by one wave in item order and the
//       slices are folded in a fixed order: bitwise repeatable, and the same whatever other chain words share the launch
//       (the slices depend on the shape and the device alone).
//   evidence_temper_kernel
//       dst = beta * src for up to EV_MAX_TABLES tables in one launch (the working tables of a rung); beta = 1 copies bit
//       for bit.
#include "fcd_common.h"

namespace {

constexpr int EV_NW = 16;          // waves per workgroup: a chain word each per pass over a staged tile
constexpr int EV_K = 2;            // passes: a workgroup serves EV_NW * EV_K chain words from one staging of the table
constexpr int EV_TI = 896;         // items per LDS tile: 63 KiB of records, two workgroups per CU (160 KiB of LDS)
constexpr int EV_MIN_ITEMS = 32;   // items per slice at least
constexpr int EV_EB = 8;           // edges whose f bytes are loaded together
constexpr int EV_MAX_TABLES = 8;

// grid (S slices, ceil(GW / (EV_NW * EV_K))), EV_NW waves.  part[s * GP + g] = the slice's sum for chain g.
__global__ __launch_bounds__(64 * EV_NW) void evidence_energy_kernel(const double *__restrict__ S_B, const double *__restrict__ lM,
                                                                     const uint8_t *__restrict__ f_state,
                                                                     const uint64_t *__restrict__ r_bits, int Nreg, int U, int64_t C,
                                                                     int GW, int S, double *__restrict__ part) {
    __shared__ double tile[EV_TI * 9];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = blockIdx.x;
    const int64_t I = C * U;
    // slice s = items [i0, i0 + len): I / S each, the first I % S one more
    const int64_t per = I / S, rem = I % S;
    const int64_t i0 = per * s + (s < rem ? s : rem);
    const int64_t len = per + (s < rem ? 1 : 0);
    const int nt = (int)((len + EV_TI - 1) / EV_TI);
    const int64_t tper = nt ? len / nt : 0, trem = nt ? len % nt : 0;
    double acc[EV_K];
#pragma unroll
    for (int k = 0; k < EV_K; ++k) acc[k] = 0.0;
    for (int t = 0; t < nt; ++t) {
        const int64_t ta = i0 + tper * t + (t < trem ? t : trem);
        const int ni = (int)(tper + (t < trem ? 1 : 0));          // <= EV_TI
        const int64_t ca = ta / U, cb = (ta + ni - 1) / U;         // first and last edge of the tile
        const int ua0 = (int)(ta - ca * U);                        // first patient of the first edge
        __syncthreads();                                           // the previous tile is read
        for (int e = threadIdx.x; e < ni * 9; e += blockDim.x) {
            const int j = e / 9, comp = e - j * 9;
            const int ir = ua0 + j;                                // item relative to (ca, u = 0)
            const int dc = ir / U;
            double v = lM[ta * 9 + e];
            if (ir - dc * U == 0) v += S_B[(ca + dc) * 3 + comp / 3];
            tile[e] = v;
        }
        __syncthreads();
        int n0, m0;
        fcd_edge_to_pair(ca, n0, m0);
#pragma unroll
        for (int k = 0; k < EV_K; ++k) {
            const int w = (blockIdx.y * EV_K + k) * EV_NW + wave;
            if (w >= GW) continue;
            const uint64_t *rw = r_bits + (int64_t)w * Nreg * U;
            const uint8_t *fw = f_state + (int64_t)w * C * 64 + lane;
            int n = n0, m = m0;
            double a = 0.0;
            for (int64_t c = ca; c <= cb; c += EV_EB) {
                uint32_t fk[EV_EB];
#pragma unroll
                for (int e = 0; e < EV_EB; ++e) fk[e] = fw[(c + e <= cb ? c + e : cb) * 64];
#pragma unroll
                for (int e = 0; e < EV_EB; ++e) {
                    const int64_t cc = c + e;
                    if (cc > cb) break;
                    const int64_t first = cc * U - ta;             // item of (cc, u = 0) relative to the tile
                    const int ua = first < 0 ? (int)(-first) : 0;
                    const int ub = first + U > ni ? (int)(ni - first) : U;
                    const int kf = (int)min(fk[e], 2u);            // (f is in {0, 1, 2}; the clamp keeps a stray byte in bounds)
                    const double *rec = tile + (first * 9 + kf * 3);
                    const uint64_t *rn = rw + (int64_t)n * U, *rm = rw + (int64_t)m * U;
                    // four items at a time: their r words, then their LDS reads, in flight together; added in item order
                    int u = ua;
                    for (; u + 4 <= ub; u += 4) {
                        uint64_t x[4], y[4];
                        double v[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            x[q] = rn[u + q];
                            y[q] = rm[u + q];
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const uint32_t l = fcd_sel_mask(fcd_sel_mask(0u, 2u, x[q] ^ y[q]), 1u, x[q] & y[q]);
                            v[q] = rec[(u + q) * 9 + l];
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q) a += v[q];
                    }
                    for (; u < ub; ++u) {
                        const uint64_t x = rn[u], y = rm[u];
                        const uint32_t l = fcd_sel_mask(fcd_sel_mask(0u, 2u, x ^ y), 1u, x & y);
                        a += rec[u * 9 + l];
                    }
                    if (++m == n) {
                        ++n;
                        m = 0;
                    }
                }
            }
            acc[k] += a;
        }
    }
    const int64_t GP = (int64_t)GW * 64;
#pragma unroll
    for (int k = 0; k < EV_K; ++k) {
        const int w = (blockIdx.y * EV_K + k) * EV_NW + wave;
        if (w < GW) part[(int64_t)s * GP + (int64_t)w * 64 + lane] = acc[k];
    }
}

// w[g] += dbeta * sum_s part[s, g].  256 threads = 64 chains x 4 quarters of the slices: a thread adds its quarter in slice
// order, eight loads in flight at a time (one load per add would be S memory round trips in a row), and the four quarters
// are added in quarter order: a fixed order that depends on S alone.
__global__ __launch_bounds__(256) void evidence_energy_fold(const double *__restrict__ part, int S, int64_t G, int64_t GP, double dbeta,
                                                            double *__restrict__ w) {
    __shared__ double red[4][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * 64 + lane;
    const int s0 = (int)((int64_t)S * q / 4), s1 = (int)((int64_t)S * (q + 1) / 4);
    double e = 0.0;
    if (g < G) {
        int s = s0;
        for (; s + 8 <= s1; s += 8) {
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = part[(int64_t)(s + j) * GP + g];
#pragma unroll
            for (int j = 0; j < 8; ++j) e += v[j];
        }
        for (; s < s1; ++s) e += part[(int64_t)s * GP + g];
    }
    red[q][lane] = e;
    __syncthreads();
    if (q == 0 && g < G) w[g] += dbeta * (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]);
}

struct temper_args {
    const double *src[EV_MAX_TABLES];
    double *dst[EV_MAX_TABLES];
    int64_t n[EV_MAX_TABLES];
};

// grid (blocks, tables): table blockIdx.y, grid-stride over its elements; pairs of doubles where both pointers allow
__global__ __launch_bounds__(256) void evidence_temper_kernel(temper_args a, double beta) {
    const double *src = nullptr;
    double *dst = nullptr;
    int64_t n = 0;
#pragma unroll
    for (int j = 0; j < EV_MAX_TABLES; ++j) {
        if (j == (int)blockIdx.y) {
            src = a.src[j];
            dst = a.dst[j];
            n = a.n[j];
        }
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t done = 0;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const double2 *s2 = reinterpret_cast<const double2 *>(src);
        double2 *d2 = reinterpret_cast<double2 *>(dst);
        const int64_t n2 = n / 2;
        for (int64_t i = i0; i < n2; i += stride) {
            double2 v = s2[i];
            v.x = beta * v.x;
            v.y = beta * v.y;
            d2[i] = v;
        }
        done = n2 * 2;
    }
    for (int64_t i = done + i0; i < n; i += stride) dst[i] = beta * src[i];
}

}  // namespace

extern "C" int fcd_evidence_energy(fcd_ctx *ctx, const double *S_B, const double *lM, const uint8_t *f_state, const uint64_t *r_bits,
                                   int64_t Nreg, int64_t U, int64_t G, double beta_prev, double beta, double *w,
                                   fcd_stream stream) {
    fcd_geo g;
    int rc = fcd_geo_check(ctx, Nreg, U, G, 0, g);
    if (rc) return rc;
    if (!S_B || !lM || !f_state || !r_bits || !w) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_evidence_energy: null pointer");
    // slices: two workgroups per CU where there are that many items; a function of the shape and the device, never of G
    const int64_t I = g.C * U;
    int64_t S = I / EV_MIN_ITEMS;
    if (S > 2 * (int64_t)ctx->num_cu) S = 2 * (int64_t)ctx->num_cu;
    if (S < 1) S = 1;
    const int64_t GP = (int64_t)g.GW * 64;
    rc = fcd_ws_reserve(ctx, (size_t)S * (size_t)GP * sizeof(double));
    if (rc) return rc;
    double *part = (double *)ctx->ws.p;
    hipStream_t s = (hipStream_t)stream;
    const int groups = (g.GW + EV_NW * EV_K - 1) / (EV_NW * EV_K);
    hipLaunchKernelGGL(evidence_energy_kernel, dim3((unsigned)S, (unsigned)groups), dim3(64 * EV_NW), 0, s, S_B, lM, f_state, r_bits,
                       (int)Nreg, (int)U, g.C, g.GW, (int)S, part);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(evidence_energy_fold, dim3((unsigned)((G + 63) / 64)), dim3(256), 0, s, (const double *)part, (int)S, G, GP,
                       beta - beta_prev, w);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_evidence_temper(fcd_ctx *ctx, double beta, int64_t n_tables, const double *const *src, double *const *dst,
                                   const int64_t *n, fcd_stream stream) {
    if (!ctx) return FCD_ERR_ARG;
    if (!src || !dst || !n) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_evidence_temper: null pointer");
    if (n_tables < 1 || n_tables > EV_MAX_TABLES)
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_evidence_temper: %lld tables (1 to %lld)", n_tables, EV_MAX_TABLES);
    temper_args a = {};
    int64_t largest = 0;
    for (int64_t j = 0; j < n_tables; ++j) {
        if (!src[j] || !dst[j] || n[j] < 0) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_evidence_temper: table %lld is null or negative", j);
        a.src[j] = src[j];
        a.dst[j] = dst[j];
        a.n[j] = n[j];
        if (n[j] > largest) largest = n[j];
    }
    if (largest == 0) return FCD_OK;
    int64_t blocks = (largest / 2 + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cu * 16;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(evidence_temper_kernel, dim3((unsigned)blocks, (unsigned)n_tables), dim3(256), 0, (hipStream_t)stream, a, beta);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
