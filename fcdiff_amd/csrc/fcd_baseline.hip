// K_base: the two classical baselines (fcd_baseline_normative, fcd_baseline_group_perm).  Not in the reference; oracle =
// tests/baseline_ref.py.  E(n) = the N - 1 connections that touch region n, walked as k = 0 .. N - 2 with the other endpoint
// m = k (k < n) or k + 1: rows tri(n) + k are contiguous for k < n, rows tri(m) + n are strided for k >= n.  A connection
// is met by both its endpoints; what is written once per connection (z, z0, n_controls, t, count_t) is written by the
// endpoint n > m.  Caller's stream, fixed reduction orders, no floating-point atomics: two calls agree bit for bit.
//
// Normative scores
//   baseline_normative_kernel   grid (N, chunks of 64 subjects), 4 waves.  A wave takes connections k = wave, wave + 4, ...:
//                      the control row goes into the wave's LDS row once; count, mean and sum of squares about the mean in two
//                      passes, lanes over the controls, butterfly sums.  Then lane = subject (controls first, then patients):
//                      a patient lane scores its bt value, a control lane takes the deleted sums of the other controls
//                      straight from the LDS row (every lane reads the same address: a broadcast) -- 2 H reads, no downdate.
//                      z^2, the count of defined scores and of |z| > threshold stay in registers over the wave's
//                      connections; the four waves meet in LDS and wave 0 adds them in wave order.
//
// Permutation group test (statistics in their t^2 form: one division per value, the root only where a t leaves the device)
//   group_centre_kernel   one wave per row of X = [b | bt]: mean over the S subjects, x - mean, Q = sum (x - mean)^2, written
//                      K-step major: XT[j][c][0..3] = subjects 4 j .. 4 j + 3 of row c, zeros behind S.
//   group_pack_kernel  the labels of 16 permutations x 128 subjects as one uint32 per lane: bit j of lane l = label of
//                      permutation l & 15 at subject 4 (32 w + j) + (l >> 4) -- what that lane feeds the MFMA as A at
//                      K-step 32 w + j.  labels == nullptr: the observed labelling (ones on the last U subjects).
//   gp_tile_mma        what the two kernels below share: a tile of 16 permutations x 16 connections over all K-steps in
//                      ascending order.  Per K-step ONE 8-byte load per lane (lane l: row of connection l & 15, subject
//                      4 j + (l >> 4) -- 512 contiguous bytes where the 16 rows are contiguous, 32-byte pieces where they are
//                      strided: the same address formula, the lane's row offset is all that differs), the label bit
//                      expanded to 0.0 / 1.0 in two VALU instructions, one v_mfma_f64_16x16x4_f64 per group.  Then
//                      gp_t2: g = A^2 S/(U H), t^2 = g (S - 2) / (Q - g).
//   Degenerate connections (pinned by tests/test_gpu_baseline_exact.py; no extra pass, no extra launch):
//     constant         all S values equal (min == max, K_cov's rule; the centre kernel compares every value it reads with the
//                      first): centred values and Q exactly 0.  t = NaN (group test and bits kernel), exactly 0 to every region
//                      sum, observed and permuted, no part in any maximum, never suprathreshold, count_t = 0.  A region whose
//                      connections are all constant has region = 0 and count_region = P.
//     separated        SS_w = Q - g not > 0 with Q > 0 (Q - g is a difference of two rounded numbers): t^2 = +inf, t = +/-inf
//                      with the sign of A; inf >= inf counts.  No other finite input gives a NaN, and no region sum ever sees
//                      a negative term.
//   group_observed_kernel   the observed labelling as one packed row: a wave per 16 consecutive connections, each connection
//                      once; writes t and t^2.  group_observed_region_kernel adds t^2 over E(n) exactly as the permutation
//                      kernel adds a row's (lane = column of the tile, tiles in order, then the butterfly).  A row of
//                      labels equal to the observed labelling therefore gives the observed statistics bit for bit: the
//                      same operations on the same numbers in the same order.  (The permutation kernel itself at P = 1
//                      did the same in 112 us at 200 regions -- 200 single waves, each 13 tiles of dependent loads long.)
//   baseline_group_kernel   grid (N, blocks of 128 permutations), 4 waves x 2 groups of 16 permutations.  A wave reads its
//                      label words once into registers (at most 2 x 8), then walks E(n) in tiles of 16 connections.
//                      Epilogue per tile: per lane a running sum and max of t^2 over the tiles (tile order), folded over
//                      the 16 lanes of a permutation by a fixed butterfly after the last tile; t^2 >= observed t^2 counted
//                      per connection (integer atomics).  Writes the (n, p) partials.
//   group_fold_kernel  workgroup n: the exceedance count of region n, threads over the permutations; the workgroups behind
//                      them: thread = permutation, max over n of both partials.  No atomics.
//
// Network-based statistic (fcd_baseline_network_bits, fcd_graph_components): threshold t, take the connected components
//   network_bits_kernel      group_centre_kernel, group_pack_kernel, gp_tile_mma and gp_t2 as above, but each connection once
//                      (half of the permutation kernel's matrix work) and nothing kept but one bit per (labelling, connection):
//                      a wave takes 16 consecutive connections x 4 groups of 16 labellings; one ballot per result element
//                      holds the 16 connections of four labellings, stored as four uint16 (plain vector stores).  The
//                      observed labelling is a call with P = 1 through the same kernel.
//                      (fcd_baseline_group_perm_opt, fcd_baseline_network_bits_opt: the same with missing data and Welch's t,
//                      kernels of their own at the end of the namespace; oracle = tests/baseline_missing_ref.py.)
//                      (fcd_baseline_group_glm, fcd_baseline_network_bits_glm: the same with nuisance covariates, the A operand a
//                      double read from the design in LDS by a permuted index; kernels of their own behind those, where they
//                      are described; oracle = tests/baseline_glm_ref.py.)
//   graph_components_kernel  one workgroup per row of bits, the row in LDS (64 KB at 1024 regions, the limit).  label[x] = x;
//                      per round every set bit (n, m) pulls the larger label, and the region that label names, down to the
//                      smaller (LDS atomicMin), then label[x] = label[label[x]]; until a round changes nothing, at most N
//                      rounds.  Then extents, regions, maxima with integer LDS atomics.
#include "fcd_common.h"

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int BN_WAVES = 4;
constexpr int BN_HMAX = 1024;            // controls of the normative kernel: one LDS row per wave
constexpr int GP_WAVES = 4, GP_G = 2;    // waves per workgroup, groups of 16 permutations per wave
constexpr int GP_PB = GP_WAVES * GP_G * 16;
constexpr int GP_SMAX = 1024;            // subjects of the group test: 8 label words of 32 K-steps per lane and group
constexpr int GP_NW = GP_SMAX / 128;

// Orders a wave's LDS traffic: what its lanes wrote before is what they read after.
__device__ __forceinline__ void bl_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int bl_wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// connection k of E(n), 0 <= k < N - 1: the other endpoint and the row
__device__ __forceinline__ int64_t bl_edge(int n, int k, int &m) {
    m = k < n ? k : k + 1;
    return n > m ? fcd_tri(n) + m : fcd_tri(m) + n;
}

struct norm_args {
    const double *b, *bt;
    int N, H, U;
    double thr;
    double *msq0, *msq;
    int32_t *ne0, *ne, *no0, *no, *n_controls;
    double *z0, *z;      // nullable
};

__global__ __launch_bounds__(64 * BN_WAVES) void baseline_normative_kernel(norm_args a) {
    __shared__ double row[BN_WAVES][BN_HMAX];
    __shared__ double red_sq[BN_WAVES][64];
    __shared__ int red_cnt[BN_WAVES][64], red_over[BN_WAVES][64];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = blockIdx.x, N = a.N, H = a.H, U = a.U;
    const int64_t j = (int64_t)blockIdx.y * 64 + lane;        // subject: controls, then patients
    const bool is_ctl = j < H, live = j < (int64_t)H + U;
    const int64_t u = j - H;
    const double nan = __builtin_nan("");
    double *rw = row[wv];
    double sq = 0.0;
    int cnt = 0, over = 0;
    for (int k = wv; k < N - 1; k += BN_WAVES) {
        int m;
        const int64_t c = bl_edge(n, k, m);
        const double *__restrict__ br = a.b + c * H;
        int nobs = 0;
        double s = 0.0;
        for (int h = lane; h < H; h += 64) {
            const double v = br[h];
            rw[h] = v;
            if (v == v) {
                ++nobs;
                s += v;
            }
        }
        nobs = bl_wave_sum_int(nobs);
        s = fcd_wave_sum(s);
        bl_wave_sync();
        const double mean = s / (double)nobs;
        double ss = 0.0;
        for (int h = lane; h < H; h += 64) {
            const double v = rw[h];
            if (v == v) {
                const double d = v - mean;
                ss += d * d;
            }
        }
        ss = fcd_wave_sum(ss);                               // (all lanes: before the subjects part ways)
        double zv = nan;
        if (nobs >= 3) {                                     // (wave-uniform)
            if (is_ctl) {
                const int hj = (int)j;
                const double x = rw[hj];
                if (x == x) {
                    // the other nobs - 1 observed controls: their sums as they stand, nothing taken off a full sum
                    double s1 = 0.0;
                    for (int q = 0; q < H; ++q) {
                        const double v = rw[q];
                        if (q != hj && v == v) s1 += v;
                    }
                    const double m1 = s1 / (double)(nobs - 1);
                    double ss1 = 0.0;
                    for (int q = 0; q < H; ++q) {
                        const double v = rw[q];
                        if (q != hj && v == v) {
                            const double d = v - m1;
                            ss1 += d * d;
                        }
                    }
                    const double sd1 = sqrt(ss1 / (double)(nobs - 2));
                    if (sd1 > 0.0) zv = (x - m1) / (sd1 * sqrt(1.0 + 1.0 / (double)(nobs - 1)));
                }
            } else if (live) {
                const double x = a.bt[c * U + u];
                const double sd = sqrt(ss / (double)(nobs - 1));
                if (x == x && sd > 0.0) zv = (x - mean) / (sd * sqrt(1.0 + 1.0 / (double)nobs));
            }
        }
        if (zv == zv) {
            sq += zv * zv;
            ++cnt;
            over += fabs(zv) > a.thr ? 1 : 0;
        }
        if (k < n) {                                         // the endpoint n > m writes what exists once per connection
            if (is_ctl) {
                if (a.z0) a.z0[c * H + j] = zv;
            } else if (live) {
                if (a.z) a.z[c * U + u] = zv;
            }
            if (blockIdx.y == 0 && lane == 0) a.n_controls[c] = nobs;
        }
        bl_wave_sync();                                      // the row is overwritten by the next connection
    }
    red_sq[wv][lane] = sq;
    red_cnt[wv][lane] = cnt;
    red_over[wv][lane] = over;
    __syncthreads();
    if (wv != 0 || !live) return;
    double tsq = 0.0;
    int tc = 0, to = 0;
#pragma unroll
    for (int w = 0; w < BN_WAVES; ++w) {
        tsq += red_sq[w][lane];
        tc += red_cnt[w][lane];
        to += red_over[w][lane];
    }
    const double msq = tc > 0 ? tsq / (double)tc : nan;
    if (is_ctl) {
        a.msq0[(int64_t)n * H + j] = msq;
        a.ne0[(int64_t)n * H + j] = tc;
        a.no0[(int64_t)n * H + j] = to;
    } else {
        a.msq[(int64_t)n * U + u] = msq;
        a.ne[(int64_t)n * U + u] = tc;
        a.no[(int64_t)n * U + u] = to;
    }
}

// ---- group test ----------------------------------------------------------------------------------------------------------

// workspace of one call: XT (KS, C, 4) | Q (C) | t2obs (C) | Rpart (N, P) | Mpart (N, P) | label words (PG, nw, 64) uint32
struct gp_ws {
    double *XT, *Q, *t2obs, *Rpart, *Mpart;
    uint32_t *LW;
};
__host__ static inline size_t gp_ws_bytes(int64_t C, int64_t N, int64_t P, int KS, int nw) {
    const int64_t PG = (P + 15) / 16;
    return (size_t)((int64_t)KS * C * 4 + 2 * C + 2 * N * P) * sizeof(double) + (size_t)(PG * nw * 64) * sizeof(uint32_t);
}
__host__ static inline gp_ws gp_ws_at(void *ws, int64_t C, int64_t N, int64_t P, int KS) {
    gp_ws o;
    o.XT = (double *)ws;
    o.Q = o.XT + (int64_t)KS * C * 4;
    o.t2obs = o.Q + C;
    o.Rpart = o.t2obs + C;
    o.Mpart = o.Rpart + N * P;
    o.LW = (uint32_t *)(o.Mpart + N * P);
    return o;
}

constexpr int GC_WAVES = 4;
__global__ __launch_bounds__(64 * GC_WAVES) void group_centre_kernel(const double *__restrict__ b, const double *__restrict__ bt,
                                                                     int64_t C, int H, int U, int KS, double *__restrict__ XT,
                                                                     double *__restrict__ Q) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t c = (int64_t)blockIdx.x * GC_WAVES + wv;
    if (c >= C) return;
    const int S = H + U;
    const double *__restrict__ br = b + c * H, *__restrict__ tr = bt + c * U;
    const double x0 = br[0];
    double s = 0.0;
    bool same = true;
    for (int i = lane; i < S; i += 64) {
        const double v = i < H ? br[i] : tr[i - H];
        s += v;
        same = same && v == x0;
    }
    const bool constant = __ballot(!same) == 0ull;           // all S values equal: centred values and Q are exactly 0
    const double mean = fcd_wave_sum(s) / (double)S;
    double q = 0.0;
    for (int i = lane; i < 4 * KS; i += 64) {
        double xc = 0.0;
        if (i < S && !constant) xc = (i < H ? br[i] : tr[i - H]) - mean;
        q += xc * xc;
        XT[((int64_t)(i >> 2) * C + c) * 4 + (i & 3)] = xc;
    }
    q = fcd_wave_sum(q);
    if (lane == 0) Q[c] = q;
}

__global__ __launch_bounds__(256) void group_pack_kernel(const uint8_t *__restrict__ labels, int64_t P, int H, int S, int nw,
                                                         uint32_t *__restrict__ LW) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, PG = (P + 15) / 16;
    if (idx >= PG * nw * 64) return;
    const int lane = (int)(idx & 63), w = (int)((idx >> 6) % nw);
    const int64_t p = ((idx >> 6) / nw) * 16 + (lane & 15);
    uint32_t word = 0;
    if (p < P) {
        for (int j = 0; j < 32; ++j) {
            const int s = 4 * (32 * w + j) + (lane >> 4);
            if (s < S) {
                const bool one = labels ? labels[p * S + s] != 0 : s >= H;
                word |= (one ? 1u : 0u) << j;
            }
        }
    }
    LW[idx] = word;
}

struct gp_args {
    gp_ws ws;
    int64_t C, P;
    int N, KS, nw;
    double kf, dof;                    // S / (U H), S - 2
    double *t;                         // the observed kernel's
    unsigned long long *count_t;       // the permutation kernel's
};

// bit j of a label word -> 0.0 / 1.0: the sign-extended bit masks the high word of 1.0
__device__ __forceinline__ double gp_label(uint32_t word, int j) {
    return __hiloint2double(__builtin_amdgcn_sbfe((int)word, (unsigned)j, 1u) & 0x3FF00000, 0);
}

// One tile: acc[g] = labels of group g (16 permutations) x 16 rows, over all KS K-steps in ascending order.  xp: this lane's
// row at subject lane >> 4 of K-step 0.  Four K-steps at a time, their loads issued together.
template <int G>
__device__ __forceinline__ void gp_tile_mma(const double *__restrict__ xp, int64_t jstride, const uint32_t (&lw)[G][GP_NW], int nw,
                                            int KS, double4_t (&acc)[G]) {
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int w = 0; w < GP_NW; ++w) {
        if (w < nw) {                                        // (uniform)
            const int jn = KS - 32 * w < 32 ? KS - 32 * w : 32;
            const double *__restrict__ xw = xp + (int64_t)(32 * w) * jstride;
            int j = 0;
            for (; j + 4 <= jn; j += 4) {
                double bv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) bv[i] = xw[(int64_t)(j + i) * jstride];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int g = 0; g < G; ++g)
                        acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(gp_label(lw[g][w], j + i), bv[i], acc[g], 0, 0, 0);
            }
            for (; j < jn; ++j) {
                const double bv = xw[(int64_t)j * jstride];
#pragma unroll
                for (int g = 0; g < G; ++g)
                    acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(gp_label(lw[g][w], j), bv, acc[g], 0, 0, 0);
            }
        }
    }
}

// t^2 from the sum A over the labelled subjects: g = A^2 S/(U H), t^2 = g (S - 2) / (Q - g).  Q - g is a difference of two
// rounded numbers: where it is not > 0 (complete separation) t^2 = +inf, never negative.  A constant connection (Q = 0) has
// t^2 = NaN; its callers give it no part in any sum, maximum, count or bit.  Two compares and two selects per value.
__device__ __forceinline__ double gp_t2(double A, double Qc, double kf, double dof) {
    const double gq = A * A * kf, den = Qc - gq;
    double t2 = gq * dof / den;
    if (!(den > 0.0)) t2 = __builtin_inf();
    if (!(Qc > 0.0)) t2 = __builtin_nan("");
    return t2;
}

// The observed labelling (the one row the pack kernel made of it): a wave per 16 consecutive connections, each connection
// once.  Row 0 of the tile is the labelling: lanes 0 .. 15, result element 0.
__global__ __launch_bounds__(64 * GP_WAVES) void group_observed_kernel(gp_args a) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t C = a.C, c0 = ((int64_t)blockIdx.x * GP_WAVES + wv) * 16;
    if (c0 >= C) return;
    const int col = lane & 15, ks = lane >> 4;
    const int64_t c = c0 + col < C ? c0 + col : C - 1;       // (a column past the last reads the last row and writes nothing)
    uint32_t lw[1][GP_NW];
#pragma unroll
    for (int w = 0; w < GP_NW; ++w) lw[0][w] = w < a.nw ? a.ws.LW[w * 64 + lane] : 0u;
    double4_t acc[1];
    gp_tile_mma<1>(a.ws.XT + c * 4 + ks, C * 4, lw, a.nw, a.KS, acc);
    if (ks == 0 && c0 + col < C) {
        const double A = acc[0][0];
        const double t2 = gp_t2(A, a.ws.Q[c], a.kf, a.dof);
        a.ws.t2obs[c] = t2;
        a.t[c] = copysign(sqrt(t2), A);
    }
}

// ... and its region sums, added up exactly as the permutation kernel adds a row's: lane = column of the tile, a running sum
// over the tiles in tile order, then the butterfly over the 16 columns.
__global__ __launch_bounds__(64) void group_observed_region_kernel(const double *__restrict__ t2obs, int N, double *__restrict__ region) {
    const int n = blockIdx.x, col = threadIdx.x & 15;
    double rs = 0.0;
    for (int k0 = 0; k0 < N - 1; k0 += 16) {
        const int k = k0 + col;
        const bool valid = k < N - 1;
        int m;
        double t2 = t2obs[bl_edge(n, valid ? k : N - 2, m)];
        if (!valid || t2 != t2) t2 = 0.0;                    // (NaN: a constant connection adds exactly 0)
        rs += t2;
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) rs += __shfl_xor(rs, o, 64);
    if (threadIdx.x == 0) region[n] = rs;
}

__global__ __launch_bounds__(64 * GP_WAVES) void baseline_group_kernel(gp_args a) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = blockIdx.x, N = a.N, nw = a.nw;
    const int64_t C = a.C, P = a.P, PG = (P + 15) / 16;
    const int64_t pg0 = ((int64_t)blockIdx.y * GP_WAVES + wv) * GP_G;
    if (pg0 >= PG) return;                                   // (no workgroup barrier below)
    const int col = lane & 15, ks = lane >> 4;
    uint32_t lw[GP_G][GP_NW];
#pragma unroll
    for (int g = 0; g < GP_G; ++g)
#pragma unroll
        for (int w = 0; w < GP_NW; ++w) lw[g][w] = (w < nw && pg0 + g < PG) ? a.ws.LW[((pg0 + g) * nw + w) * 64 + lane] : 0u;
    double rs[GP_G][4], mx[GP_G][4];
#pragma unroll
    for (int g = 0; g < GP_G; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) rs[g][r] = mx[g][r] = 0.0;
    for (int k0 = 0; k0 < N - 1; k0 += 16) {
        const int k = k0 + col;
        const bool valid = k < N - 1;
        int m;
        const int64_t c = bl_edge(n, valid ? k : N - 2, m);  // (a column past the last reads the last row and is masked)
        double4_t acc[GP_G];
        gp_tile_mma<GP_G>(a.ws.XT + c * 4 + ks, C * 4, lw, nw, a.KS, acc);
        // result element r of group g: permutation (pg0 + g) 16 + ks + 4 r, connection k0 + col
        const double Qc = a.ws.Q[c], t2o = a.ws.t2obs[c];
        const bool live = valid && Qc > 0.0;                 // a constant connection: 0 to the sums, no maximum, no count
        const bool own = live && k < n;
        int cnt = 0;
#pragma unroll
        for (int g = 0; g < GP_G; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double t2 = gp_t2(acc[g][r], Qc, a.kf, a.dof);
                if (!live) t2 = 0.0;
                rs[g][r] += t2;
                mx[g][r] = fmax(mx[g][r], t2);
                const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
                cnt += (own && p < P && t2 >= t2o) ? 1 : 0;
            }
        }
        cnt += __shfl_xor(cnt, 16, 64);
        cnt += __shfl_xor(cnt, 32, 64);
        if (own && ks == 0 && cnt) atomicAdd(&a.count_t[c], (unsigned long long)cnt);
    }
#pragma unroll
    for (int g = 0; g < GP_G; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double s = rs[g][r], v = mx[g][r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                s += __shfl_xor(s, o, 64);
                v = fmax(v, __shfl_xor(v, o, 64));
            }
            const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
            if (col == 0 && p < P) {
                a.ws.Rpart[(int64_t)n * P + p] = s;
                a.ws.Mpart[(int64_t)n * P + p] = v;
            }
        }
    }
}

// Workgroups 0 .. N - 1: the exceedance count of region blockIdx.x, threads over the permutations (integer sums, no atomics).
// The workgroups behind them: thread = permutation, the maxima over the regions of both partials.
__global__ __launch_bounds__(256) void group_fold_kernel(const double *__restrict__ Rpart, const double *__restrict__ Mpart,
                                                         const double *__restrict__ region, int N, int64_t P,
                                                         double *__restrict__ null_max_region, double *__restrict__ null_max_t,
                                                         int64_t *__restrict__ count_region) {
    __shared__ int red[4];
    if ((int)blockIdx.x < N) {
        const int n = blockIdx.x;
        const double Ro = region[n];
        const double *__restrict__ Rn = Rpart + (int64_t)n * P;
        int cnt = 0;
        for (int64_t p = threadIdx.x; p < P; p += 256) cnt += Rn[p] >= Ro ? 1 : 0;
        cnt = bl_wave_sum_int(cnt);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) count_region[n] = (int64_t)red[0] + red[1] + red[2] + red[3];
        return;
    }
    const int64_t p = (int64_t)(blockIdx.x - N) * 256 + threadIdx.x;
    if (p >= P) return;
    double mr = 0.0, mt = 0.0;
#pragma unroll 8
    for (int n = 0; n < N; ++n) {
        mr = fmax(mr, Rpart[(int64_t)n * P + p]);
        mt = fmax(mt, Mpart[(int64_t)n * P + p]);
    }
    null_max_region[p] = mr;
    null_max_t[p] = sqrt(mt);
}

// ---- network-based statistic ----------------------------------------------------------------------------------------------

constexpr int NB_G = 4;                  // groups of 16 labellings per wave of the bits kernel
constexpr int NB_NMAX = 1024;            // regions of the components kernel: a row of bits lives in LDS (64 KB at 1024)
constexpr int CC_T = 256;                // its threads

// workspace of one bits call: XT (KS, C, 4) | Q (C) | label words (PG, nw, 64) uint32
__host__ static inline size_t nb_ws_bytes(int64_t C, int64_t P, int KS, int nw) {
    return (size_t)((int64_t)KS * C * 4 + C) * sizeof(double) + (size_t)((P + 15) / 16 * nw * 64) * sizeof(uint32_t);
}

struct nb_args {
    const double *XT, *Q;
    const uint32_t *LW;
    int64_t C, P, W2;                  // W2 = 2 W: the 16-bit pieces of a row of bits
    int KS, nw, tail;
    double kf, dof, thr2;
    uint16_t *bits;
    double *t;                         // nullable: the t of labelling 0
};

// A wave: 16 consecutive connections (piece blockIdx.x * 4 + wave of a row of bits) x NB_G groups of 16 labellings, each
// connection once.  Result element r of group g in lane l: labelling (pg0 + g) 16 + (l >> 4) + 4 r, connection c0 + (l & 15),
// so the ballot of a compare holds, in its 16-bit field ks, the 16 connections of labelling (pg0 + g) 16 + ks + 4 r: lane
// 16 ks stores it.  A piece behind the last connection (C <= 32 W - 16) is written as zeros.
__global__ __launch_bounds__(64 * GP_WAVES) void network_bits_kernel(nb_args a) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t piece = (int64_t)blockIdx.x * GP_WAVES + wv;
    if (piece >= a.W2) return;                               // (no workgroup barrier below)
    const int64_t C = a.C, P = a.P, PG = (P + 15) / 16, c0 = piece * 16;
    const int64_t pg0 = (int64_t)blockIdx.y * NB_G;
    const int col = lane & 15, ks = lane >> 4;
    if (c0 >= C) {
#pragma unroll
        for (int g = 0; g < NB_G; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
                if (col == 0 && p < P) a.bits[p * a.W2 + piece] = (uint16_t)0;
            }
        }
        return;
    }
    const bool valid = c0 + col < C;
    const int64_t c = valid ? c0 + col : C - 1;              // (a column past the last reads the last row and contributes 0)
    uint32_t lw[NB_G][GP_NW];
#pragma unroll
    for (int g = 0; g < NB_G; ++g)
#pragma unroll
        for (int w = 0; w < GP_NW; ++w) lw[g][w] = (w < a.nw && pg0 + g < PG) ? a.LW[((pg0 + g) * a.nw + w) * 64 + lane] : 0u;
    double4_t acc[NB_G];
    gp_tile_mma<NB_G>(a.XT + c * 4 + ks, C * 4, lw, a.nw, a.KS, acc);
    const double Qc = a.Q[c];
#pragma unroll
    for (int g = 0; g < NB_G; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double A = acc[g][r];
            const double t2 = gp_t2(A, Qc, a.kf, a.dof);
            const bool side = a.tail == 0 || (a.tail == 1 ? A > 0.0 : A < 0.0);
            const unsigned long long mask = __ballot(valid && side && t2 > a.thr2);
            const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
            if (col == 0 && p < P) a.bits[p * a.W2 + piece] = (uint16_t)(mask >> (16 * ks));
            if (a.t && p == 0 && valid) a.t[c] = copysign(sqrt(t2), A);
        }
    }
}

// the set bits of word w of a row: (n, m) of connection 32 w by the corrected root, then moved along the word
template <typename F>
__device__ __forceinline__ void cc_for_bits(int w, uint32_t word, F f) {
    if (!word) return;
    int n, m, at = 0;
    fcd_edge_to_pair((int64_t)w * 32, n, m);
    while (word) {
        const int j = __ffs((int)word) - 1;
        word &= word - 1u;
        m += j - at;
        at = j;
        while (m >= n) {
            m -= n;
            ++n;
        }
        f(n, m);
    }
}

// One workgroup per row of bits.  LDS: the row's W words | label[N] | extent[N] | regions[N] | changed, n_edges, max_extent,
// max_regions.  label[x] <= x is always a region of x's component and only ever falls; at the fixed point of the edge step it
// is the component's smallest region.  Integer atomics only: the result does not depend on their order.
__global__ __launch_bounds__(CC_T) void graph_components_kernel(const uint32_t *__restrict__ bits, int64_t C, int N, int W,
                                                                int32_t *__restrict__ component, int32_t *__restrict__ n_edges,
                                                                int32_t *__restrict__ max_extent, int32_t *__restrict__ max_regions) {
    extern __shared__ uint32_t cc_lds[];
    uint32_t *words = cc_lds;
    int *label = (int *)(words + W), *extent = label + N, *regions = extent + N, *sc = regions + N;
    const int tid = threadIdx.x;
    const uint32_t *__restrict__ src = bits + (int64_t)blockIdx.x * W;
    const uint32_t last = (C & 31) ? (1u << (C & 31)) - 1u : ~0u;          // bits behind C are ignored
    for (int w = tid; w < W; w += CC_T) words[w] = src[w] & (w == W - 1 ? last : ~0u);
    for (int x = tid; x < N; x += CC_T) {
        label[x] = x;
        extent[x] = 0;
        regions[x] = 0;
    }
    if (tid < 4) sc[tid] = 0;
    __syncthreads();
    // At most N rounds: the minimum reaches every region of its component in N - 1 rounds even without the jumps.
    for (int round = 0; round < N; ++round) {
        int ch = 0;
        for (int w = tid; w < W; w += CC_T) {
            cc_for_bits(w, words[w], [&](int n, int m) {
                const int ln = label[n], lm = label[m];
                if (ln != lm) {
                    const int lo = ln < lm ? ln : lm, hi = ln < lm ? lm : ln;
                    atomicMin(&label[hi], lo);
                    atomicMin(&label[ln < lm ? m : n], lo);
                    ch = 1;
                }
            });
        }
        if (ch) sc[0] = 1;
        __syncthreads();
        const int changed = sc[0];
        for (int x = tid; x < N; x += CC_T) {                // pointer jumping
            const int l = label[x], ll = label[l];
            if (ll < l) atomicMin(&label[x], ll);
        }
        __syncthreads();
        if (!changed) break;                                 // (uniform: every thread read the same word between two barriers)
        if (tid == 0) sc[0] = 0;
        __syncthreads();
    }
    for (int w = tid; w < W; w += CC_T) cc_for_bits(w, words[w], [&](int n, int) { atomicAdd(&extent[label[n]], 1); });
    __syncthreads();
    for (int x = tid; x < N; x += CC_T) {
        const int l = label[x];
        if (extent[l] > 0) atomicAdd(&regions[l], 1);
    }
    __syncthreads();
    for (int x = tid; x < N; x += CC_T) {
        const int e = extent[x], l = label[x];
        if (e > 0) {
            atomicAdd(&sc[1], e);
            atomicMax(&sc[2], e);
            atomicMax(&sc[3], regions[x]);
        }
        if (component) component[(int64_t)blockIdx.x * N + x] = extent[l] > 0 ? l : -1;
    }
    __syncthreads();
    if (tid == 0) {
        n_edges[blockIdx.x] = sc[1];
        max_extent[blockIdx.x] = sc[2];
        max_regions[blockIdx.x] = sc[3];
    }
}

// ---- the two options: missing data (MISS) and Welch's t (WELCH) ------------------------------------------------------------
// Never instantiated with both off: that case is the kernels above, untouched.  Per group of 16 labellings up to three
// accumulators through the same tile product: A = L X as above (XT holds 0 at a missing subject), n1 = L M (MISS; M the 0/1
// observation mask, exact small integers in any order) and B = L X^2 (WELCH; the square of the value already loaded).
// The mask takes the label words' treatment: MW[(w C + c) 4 + ks], bit j = subject 4 (32 w + j) + ks of row c is observed,
// so a lane fetches one uint32 per 32 K-steps (256 contiguous bytes per word where the 16 rows are contiguous).
//   definedness      pooled: Q > 0, n >= 3, n1 >= 1, n0 >= 1; Welch: Q > 0, n1 >= 2, n0 >= 2.  Undefined under a labelling: 0 to
//                    the sums, no maximum, no bit, but an exceedance in count_t.  Undefined under the observed labelling:
//                    t2obs = NaN, the connection is dead (as a constant one).

constexpr int NBO_G = 2;                 // groups of 16 labellings per wave of the bits kernel with options (3 accumulators each)

// per connection, beside XT and Q: mask words, n = observed subjects, n1 of the observed labelling (observed patients)
struct gpo_conn {
    const uint32_t *MW;
    const int32_t *NN, *NO;
    double nS, nU;                     // what n and n1 are on complete data (MISS off)
};

__global__ __launch_bounds__(64 * GC_WAVES) void group_centre_missing_kernel(const double *__restrict__ b, const double *__restrict__ bt,
                                                                             int64_t C, int H, int U, int KS, int nw,
                                                                             double *__restrict__ XT, double *__restrict__ Q,
                                                                             uint32_t *__restrict__ MW, int32_t *__restrict__ NN,
                                                                             int32_t *__restrict__ NO, int64_t *__restrict__ n_controls,
                                                                             int64_t *__restrict__ n_patients) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t c = (int64_t)blockIdx.x * GC_WAVES + wv;
    if (c >= C) return;
    const int S = H + U;
    const double *__restrict__ br = b + c * H, *__restrict__ tr = bt + c * U;
    double s = 0.0, x0l = 0.0;
    int nc = 0, np = 0, first = INT32_MAX;
    bool same = true;
    for (int i = lane; i < S; i += 64) {
        const double v = i < H ? br[i] : tr[i - H];
        if (v == v) {
            s += v;
            if (i < H) ++nc; else ++np;
            if (first == INT32_MAX) {
                first = i;
                x0l = v;
            }
            same = same && v == x0l;
        }
    }
    // the first observed value of the row: every lane's values equal its own first, and that equals the row's first
    int fmin = first;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fmin = min(fmin, __shfl_xor(fmin, o, 64));
    const double x0 = __shfl(x0l, fmin & 63, 64);
    same = same && (first == INT32_MAX || x0l == x0);
    const bool constant = __ballot(!same) == 0ull;           // all observed values equal (none included): x and Q exactly 0
    nc = bl_wave_sum_int(nc);
    np = bl_wave_sum_int(np);
    const int n = nc + np;
    const double mean = fcd_wave_sum(s) / (double)n;
    double q = 0.0;
    for (int i = lane; i < 4 * KS; i += 64) {
        double xc = 0.0;
        if (i < S && !constant) {
            const double v = i < H ? br[i] : tr[i - H];
            if (v == v) xc = v - mean;
        }
        q += xc * xc;
        XT[((int64_t)(i >> 2) * C + c) * 4 + (i & 3)] = xc;
    }
    q = fcd_wave_sum(q);
    if (lane < 4 * nw) {                                     // one mask word per lane: K-word lane >> 2, subject phase lane & 3
        const int w = lane >> 2, ks = lane & 3;
        uint32_t word = 0;
        for (int j = 0; j < 32; ++j) {
            const int i = 4 * (32 * w + j) + ks;
            if (i < S) {
                const double v = i < H ? br[i] : tr[i - H];
                word |= (v == v ? 1u : 0u) << j;
            }
        }
        MW[((int64_t)w * C + c) * 4 + ks] = word;
    }
    if (lane == 0) {
        Q[c] = q;
        NN[c] = n;
        NO[c] = np;
        if (n_controls) n_controls[c] = nc;
        if (n_patients) n_patients[c] = np;
    }
}

__global__ __launch_bounds__(256) void group_fill_counts_kernel(int64_t C, int64_t H, int64_t U, int64_t *__restrict__ n_controls,
                                                                int64_t *__restrict__ n_patients) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    if (n_controls) n_controls[c] = H;
    if (n_patients) n_patients[c] = U;
}

// gp_tile_mma with the accumulators of the options.  mp: this lane's mask word of K-word 0 (MISS), wstride words to the next.
template <int G, bool MISS, bool WELCH>
__device__ __forceinline__ void gpo_tile_mma(const double *__restrict__ xp, int64_t jstride, const uint32_t *__restrict__ mp,
                                             int64_t wstride, const uint32_t (&lw)[G][GP_NW], int nw, int KS, double4_t (&acc)[G],
                                             double4_t (&accn)[G], double4_t (&accb)[G]) {
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = accn[g] = accb[g] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int w = 0; w < GP_NW; ++w) {
        if (w < nw) {                                        // (uniform)
            const int jn = KS - 32 * w < 32 ? KS - 32 * w : 32;
            const double *__restrict__ xw = xp + (int64_t)(32 * w) * jstride;
            uint32_t mw = 0u;
            if (MISS) mw = mp[(int64_t)w * wstride];
            int j = 0;
            for (; j + 4 <= jn; j += 4) {
                double bv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) bv[i] = xw[(int64_t)(j + i) * jstride];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double mv = gp_label(mw, j + i), b2 = bv[i] * bv[i];
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const double la = gp_label(lw[g][w], j + i);
                        acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(la, bv[i], acc[g], 0, 0, 0);
                        if (MISS) accn[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(la, mv, accn[g], 0, 0, 0);
                        if (WELCH) accb[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(la, b2, accb[g], 0, 0, 0);
                    }
                }
            }
            for (; j < jn; ++j) {
                const double bv = xw[(int64_t)j * jstride];
                const double mv = gp_label(mw, j), b2 = bv * bv;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const double la = gp_label(lw[g][w], j);
                    acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(la, bv, acc[g], 0, 0, 0);
                    if (MISS) accn[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(la, mv, accn[g], 0, 0, 0);
                    if (WELCH) accb[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(la, b2, accb[g], 0, 0, 0);
                }
            }
        }
    }
}

// The tile product of a wave's 16 connections.  Complete-tile shortcut: where all 16 are complete (n = S), every labelling has
// n1 = U there and the mask product is left out; the branch is wave-uniform and the results are the same bits either way
// (the counts are exact).  Returns whether accn was counted.  FCD_GPO_NO_SHORTCUT: a timing build without it.
template <int G, bool MISS, bool WELCH>
__device__ __forceinline__ bool gpo_tile(const double *__restrict__ xp, int64_t jstride, const uint32_t *__restrict__ mp, int64_t wstride,
                                         const uint32_t (&lw)[G][GP_NW], int nw, int KS, double nc, double nS, double4_t (&acc)[G],
                                         double4_t (&accn)[G], double4_t (&accb)[G]) {
#ifndef FCD_GPO_NO_SHORTCUT
    if (MISS && __ballot(nc != nS) == 0ull) {
        gpo_tile_mma<G, false, WELCH>(xp, jstride, mp, wstride, lw, nw, KS, acc, accn, accb);
        return false;
    }
#endif
    gpo_tile_mma<G, MISS, WELCH>(xp, jstride, mp, wstride, lw, nw, KS, acc, accn, accb);
    return MISS;
}

// t^2 of one value from A = sum l x, B = sum l x^2, n1 = sum l m, and the connection's n and Q; k = n / (n1 n0).
// Pooled: g = A^2 k, t^2 = g (n - 2) / (Q - g), +inf where Q - g is not > 0: gp_t2 operation for operation where n = S, n1 = U.
// Welch: SS1 = max(B - A^2/n1, 0), SS0 = max((Q - B) - A^2/n0, 0), v = SS1/(n1 (n1 - 1)) + SS0/(n0 (n0 - 1)), t^2 = (A k)^2 / v;
// v not > 0: +inf if A != 0, else 0.  def: whether the value is defined; what is returned where it is not is the caller's to drop.
template <bool WELCH>
__device__ __forceinline__ double gpo_t2(double A, double B, double n1, double n, double Qc, bool &def) {
    const double n0 = n - n1, k = n / (n1 * n0);
    if (!WELCH) {
        def = Qc > 0.0 && n >= 3.0 && n1 >= 1.0 && n0 >= 1.0;
        const double gq = A * A * k, den = Qc - gq;
        double t2 = gq * (n - 2.0) / den;
        if (!(den > 0.0)) t2 = __builtin_inf();
        return t2;
    }
    def = Qc > 0.0 && n1 >= 2.0 && n0 >= 2.0;
    const double a2 = A * A;
    double ss1 = B - a2 / n1, ss0 = (Qc - B) - a2 / n0;
    ss1 = ss1 > 0.0 ? ss1 : 0.0;
    ss0 = ss0 > 0.0 ? ss0 : 0.0;
    const double v = ss1 / (n1 * (n1 - 1.0)) + ss0 / (n0 * (n0 - 1.0)), d = A * k;
    double t2 = d * d / v;
    if (!(v > 0.0)) t2 = A != 0.0 ? __builtin_inf() : 0.0;
    return t2;
}

struct gpo_args {
    gp_args g;                         // kf and dof unused
    gpo_conn k;
};

template <bool MISS, bool WELCH>
__global__ __launch_bounds__(64 * GP_WAVES) void group_observed_opt_kernel(gpo_args a) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t C = a.g.C, c0 = ((int64_t)blockIdx.x * GP_WAVES + wv) * 16;
    if (c0 >= C) return;
    const int col = lane & 15, ks = lane >> 4;
    const int64_t c = c0 + col < C ? c0 + col : C - 1;       // (a column past the last reads the last row and writes nothing)
    uint32_t lw[1][GP_NW];
#pragma unroll
    for (int w = 0; w < GP_NW; ++w) lw[0][w] = w < a.g.nw ? a.g.ws.LW[w * 64 + lane] : 0u;
    double4_t acc[1], accn[1], accb[1];
    gpo_tile_mma<1, MISS, WELCH>(a.g.ws.XT + c * 4 + ks, C * 4, MISS ? a.k.MW + c * 4 + ks : nullptr, C * 4, lw, a.g.nw, a.g.KS, acc,
                                 accn, accb);
    if (ks == 0 && c0 + col < C) {
        const double A = acc[0][0];
        bool def;
        double t2 = gpo_t2<WELCH>(A, accb[0][0], MISS ? accn[0][0] : a.k.nU, MISS ? (double)a.k.NN[c] : a.k.nS, a.g.ws.Q[c], def);
        if (!def) t2 = __builtin_nan("");
        a.g.ws.t2obs[c] = t2;
        a.g.t[c] = copysign(sqrt(t2), A);
    }
}

template <bool MISS, bool WELCH>
__global__ __launch_bounds__(64 * GP_WAVES) void baseline_group_opt_kernel(gpo_args a) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = blockIdx.x, N = a.g.N, nw = a.g.nw;
    const int64_t C = a.g.C, P = a.g.P, PG = (P + 15) / 16;
    const int64_t pg0 = ((int64_t)blockIdx.y * GP_WAVES + wv) * GP_G;
    if (pg0 >= PG) return;                                   // (no workgroup barrier below)
    const int col = lane & 15, ks = lane >> 4;
    uint32_t lw[GP_G][GP_NW];
#pragma unroll
    for (int g = 0; g < GP_G; ++g)
#pragma unroll
        for (int w = 0; w < GP_NW; ++w) lw[g][w] = (w < nw && pg0 + g < PG) ? a.g.ws.LW[((pg0 + g) * nw + w) * 64 + lane] : 0u;
    double rs[GP_G][4], mx[GP_G][4];
#pragma unroll
    for (int g = 0; g < GP_G; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) rs[g][r] = mx[g][r] = 0.0;
    for (int k0 = 0; k0 < N - 1; k0 += 16) {
        const int k = k0 + col;
        const bool valid = k < N - 1;
        int m;
        const int64_t c = bl_edge(n, valid ? k : N - 2, m);  // (a column past the last reads the last row and is masked)
        double4_t acc[GP_G], accn[GP_G], accb[GP_G];
        const double nc = MISS ? (double)a.k.NN[c] : a.k.nS;
        const bool counted = gpo_tile<GP_G, MISS, WELCH>(a.g.ws.XT + c * 4 + ks, C * 4, MISS ? a.k.MW + c * 4 + ks : nullptr, C * 4, lw, nw,
                                                         a.g.KS, nc, a.k.nS, acc, accn, accb);
        // result element r of group g: permutation (pg0 + g) 16 + ks + 4 r, connection k0 + col
        const double Qc = a.g.ws.Q[c], t2o = a.g.ws.t2obs[c];
        const bool live = valid && t2o == t2o;               // dead under the observed labelling: 0 to the sums, no maximum, no count
        const bool own = live && k < n;
        int cnt = 0;
#pragma unroll
        for (int g = 0; g < GP_G; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bool def;
                double t2 = gpo_t2<WELCH>(acc[g][r], accb[g][r], counted ? accn[g][r] : a.k.nU, nc, Qc, def);
                const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
                cnt += (own && p < P && (!def || t2 >= t2o)) ? 1 : 0;      // a labelling that cannot be evaluated counts
                if (!live || !def) t2 = 0.0;
                rs[g][r] += t2;
                mx[g][r] = fmax(mx[g][r], t2);
            }
        }
        cnt += __shfl_xor(cnt, 16, 64);
        cnt += __shfl_xor(cnt, 32, 64);
        if (own && ks == 0 && cnt) atomicAdd(&a.g.count_t[c], (unsigned long long)cnt);
    }
#pragma unroll
    for (int g = 0; g < GP_G; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double s = rs[g][r], v = mx[g][r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                s += __shfl_xor(s, o, 64);
                v = fmax(v, __shfl_xor(v, o, 64));
            }
            const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
            if (col == 0 && p < P) {
                a.g.ws.Rpart[(int64_t)n * P + p] = s;
                a.g.ws.Mpart[(int64_t)n * P + p] = v;
            }
        }
    }
}

struct nbo_args {
    nb_args b;                         // kf and dof unused
    gpo_conn k;
};

// network_bits_kernel with the options: NBO_G groups of 16 labellings per wave.  A connection that is undefined under the observed
// labelling (from its own n, its observed patients and Q: no second pass) has no bit under any labelling.
template <bool MISS, bool WELCH>
__global__ __launch_bounds__(64 * GP_WAVES) void network_bits_opt_kernel(nbo_args a) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t piece = (int64_t)blockIdx.x * GP_WAVES + wv;
    if (piece >= a.b.W2) return;                             // (no workgroup barrier below)
    const int64_t C = a.b.C, P = a.b.P, PG = (P + 15) / 16, c0 = piece * 16;
    const int64_t pg0 = (int64_t)blockIdx.y * NBO_G;
    const int col = lane & 15, ks = lane >> 4;
    if (c0 >= C) {
#pragma unroll
        for (int g = 0; g < NBO_G; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
                if (col == 0 && p < P) a.b.bits[p * a.b.W2 + piece] = (uint16_t)0;
            }
        }
        return;
    }
    const bool valid = c0 + col < C;
    const int64_t c = valid ? c0 + col : C - 1;              // (a column past the last reads the last row and contributes 0)
    uint32_t lw[NBO_G][GP_NW];
#pragma unroll
    for (int g = 0; g < NBO_G; ++g)
#pragma unroll
        for (int w = 0; w < GP_NW; ++w) lw[g][w] = (w < a.b.nw && pg0 + g < PG) ? a.b.LW[((pg0 + g) * a.b.nw + w) * 64 + lane] : 0u;
    double4_t acc[NBO_G], accn[NBO_G], accb[NBO_G];
    const double nc = MISS ? (double)a.k.NN[c] : a.k.nS;
    const bool counted = gpo_tile<NBO_G, MISS, WELCH>(a.b.XT + c * 4 + ks, C * 4, MISS ? a.k.MW + c * 4 + ks : nullptr, C * 4, lw, a.b.nw,
                                                      a.b.KS, nc, a.k.nS, acc, accn, accb);
    const double Qc = a.b.Q[c], n1o = MISS ? (double)a.k.NO[c] : a.k.nU;
    bool alive;
    (void)gpo_t2<WELCH>(0.0, 0.0, n1o, nc, Qc, alive);       // defined under the observed labelling?
#pragma unroll
    for (int g = 0; g < NBO_G; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double A = acc[g][r];
            bool def;
            const double t2 = gpo_t2<WELCH>(A, accb[g][r], counted ? accn[g][r] : a.k.nU, nc, Qc, def);
            const bool side = a.b.tail == 0 || (a.b.tail == 1 ? A > 0.0 : A < 0.0);
            const unsigned long long mask = __ballot(valid && alive && def && side && t2 > a.b.thr2);
            const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
            if (col == 0 && p < P) a.b.bits[p * a.b.W2 + piece] = (uint16_t)(mask >> (16 * ks));
            if (a.b.t && p == 0 && valid) a.b.t[c] = (alive && def) ? copysign(sqrt(t2), A) : __builtin_nan("");
        }
    }
}

// what the two calls with options check alike; who = the call's name
__host__ static int gpo_check(fcd_ctx *ctx, const char *who, int64_t C, int64_t H, int64_t U, int64_t P, int flags) {
    if (C < 1 || H < 1 || U < 1 || P < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "C, H, U=%lld and P=%lld must be >= 1", U, P);
    if (flags & ~(FCD_BASELINE_MISSING | FCD_BASELINE_WELCH)) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "unknown flags 0x%llx", flags);
    if (H + U < 3) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "%lld subjects, a pooled variance needs 3", H + U);
    if ((flags & FCD_BASELINE_WELCH) && (H < 2 || U < 2))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "welch: H=%lld and U=%lld must be >= 2, a variance per group", H, U);
    if (fcd_C_to_N(C) < 2) return fcd_fail_who(ctx, FCD_ERR_SHAPE, who, "C=%lld is not a triangular number", C);
    if (H + U > GP_SMAX) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "%lld subjects, at most %lld", H + U, GP_SMAX);
    return FCD_OK;
}

// XT (KS, C, 4) | Q (C) | ... the caller's ... ; behind everything: MW (nw, C, 4) uint32 | NN (C) int32 | NO (C) int32
__host__ static inline size_t gpo_conn_bytes(int64_t C, int nw) { return (size_t)((int64_t)nw * C * 4 + 2 * C) * sizeof(uint32_t); }

#define GPO_DISPATCH(kern, flags, ...)                                                                     \
    do {                                                                                                   \
        if ((flags) == FCD_BASELINE_MISSING) hipLaunchKernelGGL((kern<true, false>), __VA_ARGS__);        \
        else if ((flags) == FCD_BASELINE_WELCH) hipLaunchKernelGGL((kern<false, true>), __VA_ARGS__);     \
        else hipLaunchKernelGGL((kern<true, true>), __VA_ARGS__);                                          \
    } while (0)

// ---- nuisance covariates: the permutation GLM of Freedman & Lane ------------------------------------------------------------
// fcd_baseline_group_glm, fcd_baseline_network_bits_glm; oracle = tests/baseline_glm_ref.py.  The design W (S, R) is orthonormal,
// every column orthogonal to the constant; column 0 is tested given the others.  Per connection e = the residuals of the row on
// [1, w_1 .. w_{R-1}], Q_e = sum e^2; per permutation pi, d_q = sum_s W[pi[s], q] e_s, t^2 = d_0^2 dof / (Q_e - sum_q d_q^2),
// dof = S - R - 1, the sign of t that of d_0.  The A operand of the MFMA is no longer a bit but a double picked by an index:
//   glm_centre_kernel  group_centre_kernel with the residualisation: columns 1 .. R - 1 of W in LDS (column-major), the mean, the
//                      R - 1 coefficients a_q = sum w_q (x - mean) as wave sums, q ascending, then e = (x - mean) - sum_q w_q a_q
//                      (q ascending), Q_e and Q_c = sum (x - mean)^2.  Writes XT exactly as group_centre_kernel does.  Dead rows
//                      (e and Q exactly 0): constant ones (min == max), and those with Q_e <= dead2 Q_c, dead2 =
//                      (8 S R 2^-52)^2: a row that is a linear function of the covariates to rounding (derivation: DESIGN.md).
//   glm_pack_kernel    the indices of 16 permutations x 4 K-steps as four uint16 in one uint64 per lane: field i of lane l of
//                      quad j4 = perms[16 pg + (l & 15)][4 (4 j4 + i) + (l >> 4)], what that lane feeds the MFMA as the row of
//                      W at K-step 4 j4 + i.  S -- a row of zeros behind W in LDS -- behind the last subject, behind the last
//                      permutation and for an index that is out of range.  perms == nullptr: the identity.
//   glm_tile_mma       W as (S + 1, RT) rows in the workgroup's LDS, RT = 2, 3, 5 or 9 >= R, zero columns behind R.  Per
//                      K-step the B value is loaded once (gp_tile_mma's addressing) and feeds all RT MFMAs of every group;
//                      per group one 8-byte index load per four K-steps, per MFMA one 8-byte LDS read at the lane's own row.
//   glm_t2             gp_t2 on (d_0, sum_q d_q^2, Q_e, dof), under the same guards.
//   glm_observed_kernel, glm_group_kernel, glm_bits_kernel   group_observed_kernel, baseline_group_kernel and
//                      network_bits_kernel around that tile product: the same running sums and maxima in tile order, the same
//                      butterfly, integer atomics by the endpoint n > m, one ballot per (group, element).  The observed
//                      statistics are the identity permutation through the same product, so a row of perms equal to the
//                      identity gives them bit for bit.  group_observed_region_kernel and group_fold_kernel are reused.

constexpr int GL_G = 2;                  // groups of 16 permutations per wave, both kernels: GL_G * RT accumulators of 8 VGPRs
constexpr int GL_RMAX = 9;

__global__ __launch_bounds__(64 * GC_WAVES) void glm_centre_kernel(const double *__restrict__ b, const double *__restrict__ bt, int64_t C,
                                                                   int H, int U, int KS, const double *__restrict__ design, int R,
                                                                   double dead2, double *__restrict__ XT, double *__restrict__ Q) {
    extern __shared__ double gl_wc[];                        // column q >= 1 of W at gl_wc[(q - 1) S + s]
    const int S = H + U;
    for (int i = threadIdx.x; i < (R - 1) * S; i += 64 * GC_WAVES) gl_wc[i] = design[(int64_t)(i % S) * R + (i / S + 1)];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t c = (int64_t)blockIdx.x * GC_WAVES + wv;
    if (c >= C) return;                                      // (no workgroup barrier below)
    const double *__restrict__ br = b + c * H, *__restrict__ tr = bt + c * U;
    const double x0 = br[0];
    double s = 0.0;
    bool same = true;
    for (int i = lane; i < S; i += 64) {
        const double v = i < H ? br[i] : tr[i - H];
        s += v;
        same = same && v == x0;
    }
    const bool constant = __ballot(!same) == 0ull;           // all S values equal: centred values and Q are exactly 0
    const double mean = fcd_wave_sum(s) / (double)S;
    double a[GL_RMAX - 1];
#pragma unroll
    for (int q = 0; q < GL_RMAX - 1; ++q) {
        a[q] = 0.0;
        if (q < R - 1) {                                     // (uniform)
            double d = 0.0;
            for (int i = lane; i < S; i += 64) {
                const double xc = constant ? 0.0 : (i < H ? br[i] : tr[i - H]) - mean;
                d += gl_wc[q * S + i] * xc;
            }
            a[q] = fcd_wave_sum(d);
        }
    }
    double qe = 0.0, qc = 0.0;
    for (int i = lane; i < 4 * KS; i += 64) {
        double xc = 0.0, e = 0.0;
        if (i < S && !constant) {
            xc = (i < H ? br[i] : tr[i - H]) - mean;
            e = xc;
#pragma unroll
            for (int q = 0; q < GL_RMAX - 1; ++q)
                if (q < R - 1) e -= gl_wc[q * S + i] * a[q];
        }
        qe += e * e;
        qc += xc * xc;
        XT[((int64_t)(i >> 2) * C + c) * 4 + (i & 3)] = e;
    }
    qe = fcd_wave_sum(qe);
    qc = fcd_wave_sum(qc);
    const bool dead = !(qe > dead2 * qc);                    // constant (0 > 0), or nothing left beside the covariates
    if (dead)
        for (int i = lane; i < 4 * KS; i += 64) XT[((int64_t)(i >> 2) * C + c) * 4 + (i & 3)] = 0.0;
    if (lane == 0) Q[c] = dead ? 0.0 : qe;
}

__global__ __launch_bounds__(256) void glm_pack_kernel(const uint16_t *__restrict__ perms, int64_t P, int S, int KS4,
                                                       uint64_t *__restrict__ PI) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, PG = (P + 15) / 16;
    if (idx >= PG * KS4 * 64) return;
    const int lane = (int)(idx & 63), j4 = (int)((idx >> 6) % KS4);
    const int64_t p = ((idx >> 6) / KS4) * 16 + (lane & 15);
    uint64_t word = 0;
    for (int i = 0; i < 4; ++i) {
        const int s = 4 * (4 * j4 + i) + (lane >> 4);
        uint32_t v = (uint32_t)S;
        if (p < P && s < S) {
            v = perms ? (uint32_t)perms[p * S + s] : (uint32_t)s;
            if (v > (uint32_t)S) v = (uint32_t)S;
        }
        word |= (uint64_t)v << (16 * i);
    }
    PI[idx] = word;
}

// W into the workgroup's LDS as (S + 1, RT) rows: zero columns behind R, a row of zeros behind S.  Ends with a barrier.
template <int RT>
__device__ __forceinline__ void glm_load_design(const double *__restrict__ design, int S, int R, double *wl) {
    for (int i = threadIdx.x; i < (S + 1) * RT; i += 64 * GP_WAVES) {
        const int s = i / RT, q = i - s * RT;
        wl[i] = (s < S && q < R) ? design[(int64_t)s * R + q] : 0.0;
    }
    __syncthreads();
}

// One tile: acc[g][q] = column q of W, permuted as group g's 16 permutations have it, x 16 rows, over all KS K-steps in
// ascending order; KS is a multiple of 4 here (the centre kernel writes zeros behind S, the pack kernel the zero row).  xp as in gp_tile_mma; ip[g]: this lane's index word of quad 0 of group g, 64 words to the next quad.
template <int RT, int G>
__device__ __forceinline__ void glm_tile_mma(const double *__restrict__ xp, int64_t jstride, const uint64_t *(&ip)[G],
                                             const double *wl, int KS, double4_t (&acc)[G][RT]) {
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int q = 0; q < RT; ++q) acc[g][q] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int j4 = 0; j4 < (KS >> 2); ++j4) {
        uint64_t iw[G];
#pragma unroll
        for (int g = 0; g < G; ++g) iw[g] = ip[g][(int64_t)j4 * 64];
        const double *__restrict__ xw = xp + (int64_t)(4 * j4) * jstride;
        double bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bv[i] = xw[(int64_t)i * jstride];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const double *row = wl + (uint32_t)((iw[g] >> (16 * i)) & 0xFFFFu) * RT;
#pragma unroll
                for (int q = 0; q < RT; ++q) acc[g][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[q], bv[i], acc[g][q], 0, 0, 0);
            }
            // the LDS reads of one K-step at a time: hoisted over all four they cost 8 G RT registers more (scratch at RT = 9)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// t^2 of result element r from d_q = acc[q][r]: t^2 = d_0^2 dof / (Q_e - sum_q d_q^2), the sum over q ascending.  gp_t2's
// guards: +inf where the denominator is not > 0, NaN for a dead connection (Q_e = 0).
template <int RT>
__device__ __forceinline__ double glm_t2(const double4_t (&d)[RT], int r, double Qe, double dof) {
    double ss = 0.0;
#pragma unroll
    for (int q = 0; q < RT; ++q) ss += d[q][r] * d[q][r];
    const double den = Qe - ss;
    double t2 = d[0][r] * d[0][r] * dof / den;
    if (!(den > 0.0)) t2 = __builtin_inf();
    if (!(Qe > 0.0)) t2 = __builtin_nan("");
    return t2;
}

struct glm_args {
    gp_ws ws;                          // LW unused
    const uint64_t *PI;
    const double *design;
    int64_t C, P;
    int N, KS, S, R;
    double dof;
    double *t;                         // the observed kernel's
    unsigned long long *count_t;       // the permutation kernel's
};

template <int RT>
__global__ __launch_bounds__(64 * GP_WAVES) void glm_observed_kernel(glm_args a) {
    extern __shared__ double gl_w[];
    glm_load_design<RT>(a.design, a.S, a.R, gl_w);
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t C = a.C, c0 = ((int64_t)blockIdx.x * GP_WAVES + wv) * 16;
    if (c0 >= C) return;                                     // (no workgroup barrier below)
    const int col = lane & 15, ks = lane >> 4;
    const int64_t c = c0 + col < C ? c0 + col : C - 1;       // (a column past the last reads the last row and writes nothing)
    const uint64_t *ip[1] = {a.PI + lane};
    double4_t acc[1][RT];
    glm_tile_mma<RT, 1>(a.ws.XT + c * 4 + ks, C * 4, ip, gl_w, a.KS, acc);
    if (ks == 0 && c0 + col < C) {
        const double t2 = glm_t2<RT>(acc[0], 0, a.ws.Q[c], a.dof);
        a.ws.t2obs[c] = t2;
        a.t[c] = copysign(sqrt(t2), acc[0][0][0]);
    }
}

template <int RT>
__global__ __launch_bounds__(64 * GP_WAVES) void glm_group_kernel(glm_args a) {
    extern __shared__ double gl_w[];
    glm_load_design<RT>(a.design, a.S, a.R, gl_w);
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = blockIdx.x, N = a.N, KS4 = a.KS >> 2;
    const int64_t C = a.C, P = a.P, PG = (P + 15) / 16;
    const int64_t pg0 = ((int64_t)blockIdx.y * GP_WAVES + wv) * GL_G;
    if (pg0 >= PG) return;                                   // (no workgroup barrier below)
    const int col = lane & 15, ks = lane >> 4;
    const uint64_t *ip[GL_G];
#pragma unroll
    for (int g = 0; g < GL_G; ++g) ip[g] = a.PI + (pg0 + g < PG ? pg0 + g : PG - 1) * KS4 * 64 + lane;      // (behind the last: masked)
    double rs[GL_G][4], mx[GL_G][4];
#pragma unroll
    for (int g = 0; g < GL_G; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) rs[g][r] = mx[g][r] = 0.0;
    for (int k0 = 0; k0 < N - 1; k0 += 16) {
        const int k = k0 + col;
        const bool valid = k < N - 1;
        int m;
        const int64_t c = bl_edge(n, valid ? k : N - 2, m);  // (a column past the last reads the last row and is masked)
        double4_t acc[GL_G][RT];
        glm_tile_mma<RT, GL_G>(a.ws.XT + c * 4 + ks, C * 4, ip, gl_w, a.KS, acc);
        // result element r of group g: permutation (pg0 + g) 16 + ks + 4 r, connection k0 + col
        const double Qc = a.ws.Q[c], t2o = a.ws.t2obs[c];
        const bool live = valid && Qc > 0.0;                 // a dead connection: 0 to the sums, no maximum, no count
        const bool own = live && k < n;
        int cnt = 0;
#pragma unroll
        for (int g = 0; g < GL_G; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double t2 = glm_t2<RT>(acc[g], r, Qc, a.dof);
                if (!live) t2 = 0.0;
                rs[g][r] += t2;
                mx[g][r] = fmax(mx[g][r], t2);
                const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
                cnt += (own && p < P && t2 >= t2o) ? 1 : 0;
            }
        }
        cnt += __shfl_xor(cnt, 16, 64);
        cnt += __shfl_xor(cnt, 32, 64);
        if (own && ks == 0 && cnt) atomicAdd(&a.count_t[c], (unsigned long long)cnt);
    }
#pragma unroll
    for (int g = 0; g < GL_G; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double s = rs[g][r], v = mx[g][r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                s += __shfl_xor(s, o, 64);
                v = fmax(v, __shfl_xor(v, o, 64));
            }
            const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
            if (col == 0 && p < P) {
                a.ws.Rpart[(int64_t)n * P + p] = s;
                a.ws.Mpart[(int64_t)n * P + p] = v;
            }
        }
    }
}

struct glm_bits_args {
    const double *XT, *Q, *design;
    const uint64_t *PI;
    int64_t C, P, W2;                  // W2 = 2 W: the 16-bit pieces of a row of bits
    int KS, S, R, tail;
    double dof, thr2;
    uint16_t *bits;
    double *t;                         // nullable: the t of permutation 0
};

// network_bits_kernel's layout of waves, ballots and stores, GL_G groups of 16 permutations per wave.
template <int RT>
__global__ __launch_bounds__(64 * GP_WAVES) void glm_bits_kernel(glm_bits_args a) {
    extern __shared__ double gl_w[];
    glm_load_design<RT>(a.design, a.S, a.R, gl_w);
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t piece = (int64_t)blockIdx.x * GP_WAVES + wv;
    if (piece >= a.W2) return;                               // (no workgroup barrier below)
    const int64_t C = a.C, P = a.P, PG = (P + 15) / 16, c0 = piece * 16;
    const int64_t pg0 = (int64_t)blockIdx.y * GL_G;
    const int col = lane & 15, ks = lane >> 4, KS4 = a.KS >> 2;
    if (c0 >= C) {
#pragma unroll
        for (int g = 0; g < GL_G; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
                if (col == 0 && p < P) a.bits[p * a.W2 + piece] = (uint16_t)0;
            }
        }
        return;
    }
    const bool valid = c0 + col < C;
    const int64_t c = valid ? c0 + col : C - 1;              // (a column past the last reads the last row and contributes 0)
    const uint64_t *ip[GL_G];
#pragma unroll
    for (int g = 0; g < GL_G; ++g) ip[g] = a.PI + (pg0 + g < PG ? pg0 + g : PG - 1) * KS4 * 64 + lane;      // (behind the last: masked)
    double4_t acc[GL_G][RT];
    glm_tile_mma<RT, GL_G>(a.XT + c * 4 + ks, C * 4, ip, gl_w, a.KS, acc);
    const double Qc = a.Q[c];
#pragma unroll
    for (int g = 0; g < GL_G; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double d0 = acc[g][0][r];
            const double t2 = glm_t2<RT>(acc[g], r, Qc, a.dof);
            const bool side = a.tail == 0 || (a.tail == 1 ? d0 > 0.0 : d0 < 0.0);
            const unsigned long long mask = __ballot(valid && side && t2 > a.thr2);
            const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
            if (col == 0 && p < P) a.bits[p * a.W2 + piece] = (uint16_t)(mask >> (16 * ks));
            if (a.t && p == 0 && valid) a.t[c] = copysign(sqrt(t2), d0);
        }
    }
}

// what the two calls with a design check alike; who = the call's name
__host__ static int glm_check(fcd_ctx *ctx, const char *who, int64_t C, int64_t H, int64_t U, int64_t R, int64_t P) {
    if (C < 1 || H < 1 || U < 1 || P < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "C, H, U=%lld and P=%lld must be >= 1", U, P);
    if (R < 1 || R > GL_RMAX) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "R=%lld design columns, 1 to %lld", R, GL_RMAX);
    if (H + U > GP_SMAX) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "%lld subjects, at most %lld", H + U, GP_SMAX);
    if (H + U < R + 2) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "%lld subjects, R=%lld design columns need R + 2", H + U, R);
    if (fcd_C_to_N(C) < 2) return fcd_fail_who(ctx, FCD_ERR_SHAPE, who, "C=%lld is not a triangular number", C);
    return FCD_OK;
}

__host__ static inline int glm_width(int R) { return R <= 2 ? 0 : R <= 3 ? 1 : R <= 5 ? 2 : 3; }      // RT = 2, 3, 5, 9
__host__ static inline double glm_dead2(int64_t S, int64_t R) {
    const double tol = 8.0 * (double)S * (double)R * 2.220446049250313e-16;
    return tol * tol;
}

// kern<RT> with (S + 1) RT doubles of dynamic LDS, its limit raised where that is more than 64 KB; which = 0, 1, 2 of FCD_KA_GLM
#define GLM_LAUNCH_RT(kern, RT, which, grid, st, arg)                                                                              \
    do {                                                                                                                           \
        const size_t shmem__ = (size_t)((arg).S + 1) * (RT) * sizeof(double);                                                      \
        int rc__ = fcd_lds_attr(ctx, FCD_KA_GLM + 4 * (which) + glm_width(RT), reinterpret_cast<const void *>(&kern<RT>), shmem__); \
        if (rc__) return rc__;                                                                                                     \
        hipLaunchKernelGGL((kern<RT>), grid, dim3(64 * GP_WAVES), shmem__, st, arg);                                               \
    } while (0)
#define GLM_LAUNCH(kern, which, grid, st, arg)                               \
    do {                                                                     \
        switch (glm_width((arg).R)) {                                        \
        case 0: GLM_LAUNCH_RT(kern, 2, which, grid, st, arg); break;         \
        case 1: GLM_LAUNCH_RT(kern, 3, which, grid, st, arg); break;         \
        case 2: GLM_LAUNCH_RT(kern, 5, which, grid, st, arg); break;         \
        default: GLM_LAUNCH_RT(kern, 9, which, grid, st, arg); break;        \
        }                                                                    \
        FCD_LAUNCH_CHECK();                                                  \
    } while (0)

}  // namespace

extern "C" int fcd_baseline_normative(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                      double z_threshold, double *msq0, int32_t *n_edges0, int32_t *n_over0, double *msq,
                                      int32_t *n_edges, int32_t *n_over, int32_t *n_controls, double *z0, double *z,
                                      fcd_stream stream) {
    if (!ctx || !b || !bt || !msq0 || !n_edges0 || !n_over0 || !msq || !n_edges || !n_over || !n_controls)
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_baseline_normative: null pointer");
    if (C < 1 || H < 1 || U < 1) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_baseline_normative: C, H=%lld and U=%lld must be >= 1", H, U);
    const int64_t N = fcd_C_to_N(C);
    if (N < 2) return fcd_fail(ctx, FCD_ERR_SHAPE, "fcd_baseline_normative: C=%lld is not a triangular number", C);
    if (H > BN_HMAX) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_baseline_normative: H=%lld controls, at most %lld", H, BN_HMAX);
    const int64_t gy = (H + U + 63) / 64;
    if (N > 46340 || gy > 65535)
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_baseline_normative: shape too large (Nreg=%lld, U=%lld)", N, U);
    norm_args a;
    a.b = b;
    a.bt = bt;
    a.N = (int)N;
    a.H = (int)H;
    a.U = (int)U;
    a.thr = z_threshold;
    a.msq0 = msq0;
    a.msq = msq;
    a.ne0 = n_edges0;
    a.ne = n_edges;
    a.no0 = n_over0;
    a.no = n_over;
    a.n_controls = n_controls;
    a.z0 = z0;
    a.z = z;
    hipLaunchKernelGGL(baseline_normative_kernel, dim3((unsigned)N, (unsigned)gy), dim3(64 * BN_WAVES), 0, (hipStream_t)stream, a);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_baseline_group_perm(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                       const uint8_t *labels, int64_t P, double *t, double *region, double *null_max_t,
                                       double *null_max_region, int64_t *count_t, int64_t *count_region, fcd_stream stream) {
    if (!ctx || !b || !bt || !labels || !t || !region || !null_max_t || !null_max_region || !count_t || !count_region)
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_baseline_group_perm: null pointer");
    if (C < 1 || H < 1 || U < 1 || P < 1)
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_baseline_group_perm: C, H, U=%lld and P=%lld must be >= 1", U, P);
    const int64_t S = H + U;
    if (S < 3) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_baseline_group_perm: %lld subjects, a pooled variance needs 3", S);
    const int64_t N = fcd_C_to_N(C);
    if (N < 2) return fcd_fail(ctx, FCD_ERR_SHAPE, "fcd_baseline_group_perm: C=%lld is not a triangular number", C);
    if (S > GP_SMAX) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_baseline_group_perm: %lld subjects, at most %lld", S, GP_SMAX);
    const int64_t gy = (P + GP_PB - 1) / GP_PB;
    if (N > 46340 || gy > 65535 || (C + GC_WAVES - 1) / GC_WAVES > INT32_MAX || N * P > (1ll << 34))
        return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_baseline_group_perm: shape too large (Nreg=%lld, P=%lld)", N, P);
    const int KS = (int)((S + 3) / 4), nw = (KS + 31) / 32;
    hipStream_t st = (hipStream_t)stream;
    // Nothing of the workspace outlives the call.
    int rc = fcd_ws_reserve(ctx, gp_ws_bytes(C, N, P, KS, nw));
    if (rc) return rc;
    gp_args a;
    a.ws = gp_ws_at(ctx->ws, C, N, P, KS);
    a.C = C;
    a.N = (int)N;
    a.KS = KS;
    a.nw = nw;
    a.kf = (double)S / ((double)U * (double)H);
    a.dof = (double)(S - 2);
    a.t = t;
    a.count_t = reinterpret_cast<unsigned long long *>(count_t);
    FCD_HIP_TRY(hipMemsetAsync(count_t, 0, (size_t)C * sizeof(int64_t), st));
    hipLaunchKernelGGL(group_centre_kernel, dim3((unsigned)((C + GC_WAVES - 1) / GC_WAVES)), dim3(64 * GC_WAVES), 0, st, b, bt, C, (int)H,
                       (int)U, KS, a.ws.XT, a.ws.Q);
    FCD_LAUNCH_CHECK();
    // the observed labelling: one packed row through the same tile product and the same t^2, each connection once
    a.P = 1;
    hipLaunchKernelGGL(group_pack_kernel, dim3((unsigned)((nw * 64 + 255) / 256)), dim3(256), 0, st, (const uint8_t *)nullptr, (int64_t)1,
                       (int)H, (int)S, nw, a.ws.LW);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(group_observed_kernel, dim3((unsigned)((C + 16 * GP_WAVES - 1) / (16 * GP_WAVES))), dim3(64 * GP_WAVES), 0, st, a);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(group_observed_region_kernel, dim3((unsigned)N), dim3(64), 0, st, a.ws.t2obs, (int)N, region);
    FCD_LAUNCH_CHECK();
    a.P = P;
    const int64_t PG = (P + 15) / 16;
    hipLaunchKernelGGL(group_pack_kernel, dim3((unsigned)((PG * nw * 64 + 255) / 256)), dim3(256), 0, st, labels, P, (int)H, (int)S, nw,
                       a.ws.LW);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(baseline_group_kernel, dim3((unsigned)N, (unsigned)gy), dim3(64 * GP_WAVES), 0, st, a);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(group_fold_kernel, dim3((unsigned)(N + (P + 255) / 256)), dim3(256), 0, st, a.ws.Rpart, a.ws.Mpart, region, (int)N, P,
                       null_max_region, null_max_t, count_region);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_baseline_network_bits(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                         const uint8_t *labels, int64_t P, double threshold, int tail, uint32_t *bits, double *t,
                                         fcd_stream stream) {
    if (!ctx || !b || !bt || !bits) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_baseline_network_bits: null pointer");
    if (C < 1 || H < 1 || U < 1 || P < 1)
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_baseline_network_bits: C, H, U=%lld and P=%lld must be >= 1", U, P);
    if (!labels && P != 1) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_baseline_network_bits: the observed labelling (labels == NULL) is P = 1, not %lld", P);
    if (!(threshold > 0.0) || !(threshold <= 1.7976931348623157e308))
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_baseline_network_bits: the threshold must be finite and > 0");
    if (tail < FCD_TAIL_BOTH || tail > FCD_TAIL_LESS) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_baseline_network_bits: unknown tail %lld", tail);
    const int64_t S = H + U;
    if (S < 3) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_baseline_network_bits: %lld subjects, a pooled variance needs 3", S);
    const int64_t N = fcd_C_to_N(C);
    if (N < 2) return fcd_fail(ctx, FCD_ERR_SHAPE, "fcd_baseline_network_bits: C=%lld is not a triangular number", C);
    if (N > NB_NMAX) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_baseline_network_bits: %lld regions, at most %lld", N, NB_NMAX);
    if (S > GP_SMAX) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_baseline_network_bits: %lld subjects, at most %lld", S, GP_SMAX);
    const int64_t PG = (P + 15) / 16, gy = (PG + NB_G - 1) / NB_G, W = (C + 31) / 32;
    if (gy > 65535) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_baseline_network_bits: shape too large (Nreg=%lld, P=%lld)", N, P);
    const int KS = (int)((S + 3) / 4), nw = (KS + 31) / 32;
    hipStream_t st = (hipStream_t)stream;
    // Nothing of the workspace outlives the call.
    int rc = fcd_ws_reserve(ctx, nb_ws_bytes(C, P, KS, nw));
    if (rc) return rc;
    double *XT = (double *)ctx->ws, *Q = XT + (int64_t)KS * C * 4;
    uint32_t *LW = (uint32_t *)(Q + C);
    hipLaunchKernelGGL(group_centre_kernel, dim3((unsigned)((C + GC_WAVES - 1) / GC_WAVES)), dim3(64 * GC_WAVES), 0, st, b, bt, C, (int)H,
                       (int)U, KS, XT, Q);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(group_pack_kernel, dim3((unsigned)((PG * nw * 64 + 255) / 256)), dim3(256), 0, st, labels, P, (int)H, (int)S, nw, LW);
    FCD_LAUNCH_CHECK();
    nb_args a;
    a.XT = XT;
    a.Q = Q;
    a.LW = LW;
    a.C = C;
    a.P = P;
    a.W2 = 2 * W;
    a.KS = KS;
    a.nw = nw;
    a.tail = tail;
    a.kf = (double)S / ((double)U * (double)H);
    a.dof = (double)(S - 2);
    a.thr2 = threshold * threshold;
    a.bits = reinterpret_cast<uint16_t *>(bits);
    a.t = t;
    hipLaunchKernelGGL(network_bits_kernel, dim3((unsigned)((2 * W + GP_WAVES - 1) / GP_WAVES), (unsigned)gy), dim3(64 * GP_WAVES), 0, st, a);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_baseline_group_perm_opt(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                           const uint8_t *labels, int64_t P, int flags, double *t, double *region, double *null_max_t,
                                           double *null_max_region, int64_t *count_t, int64_t *count_region, int64_t *n_controls,
                                           int64_t *n_patients, fcd_stream stream) {
    const char *who = "fcd_baseline_group_perm_opt";
    if (!ctx || !b || !bt || !labels || !t || !region || !null_max_t || !null_max_region || !count_t || !count_region)
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    int rc = gpo_check(ctx, who, C, H, U, P, flags);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!flags) {                                            // no option: the call without them, and the counts it implies
        rc = fcd_baseline_group_perm(ctx, b, bt, C, H, U, labels, P, t, region, null_max_t, null_max_region, count_t, count_region, stream);
        if (rc || (!n_controls && !n_patients)) return rc;
        hipLaunchKernelGGL(group_fill_counts_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, C, H, U, n_controls, n_patients);
        FCD_LAUNCH_CHECK();
        return FCD_OK;
    }
    const int64_t S = H + U, N = fcd_C_to_N(C);
    const int64_t gy = (P + GP_PB - 1) / GP_PB;
    if (N > 46340 || gy > 65535 || (C + GC_WAVES - 1) / GC_WAVES > INT32_MAX || N * P > (1ll << 34))
        return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "shape too large (Nreg=%lld, P=%lld)", N, P);
    const int KS = (int)((S + 3) / 4), nw = (KS + 31) / 32;
    const bool miss = flags & FCD_BASELINE_MISSING;
    // Nothing of the workspace outlives the call.
    const size_t base = gp_ws_bytes(C, N, P, KS, nw);
    rc = fcd_ws_reserve(ctx, base + gpo_conn_bytes(C, nw));
    if (rc) return rc;
    gpo_args a;
    a.g.ws = gp_ws_at(ctx->ws, C, N, P, KS);
    uint32_t *MW = (uint32_t *)((char *)ctx->ws + base);
    int32_t *NN = (int32_t *)(MW + (int64_t)nw * C * 4), *NO = NN + C;
    a.k.MW = MW;
    a.k.NN = NN;
    a.k.NO = NO;
    a.k.nS = (double)S;
    a.k.nU = (double)U;
    a.g.C = C;
    a.g.N = (int)N;
    a.g.KS = KS;
    a.g.nw = nw;
    a.g.kf = 0.0;
    a.g.dof = 0.0;
    a.g.t = t;
    a.g.count_t = reinterpret_cast<unsigned long long *>(count_t);
    FCD_HIP_TRY(hipMemsetAsync(count_t, 0, (size_t)C * sizeof(int64_t), st));
    const dim3 gc((unsigned)((C + GC_WAVES - 1) / GC_WAVES));
    if (miss) {
        hipLaunchKernelGGL(group_centre_missing_kernel, gc, dim3(64 * GC_WAVES), 0, st, b, bt, C, (int)H, (int)U, KS, nw, a.g.ws.XT, a.g.ws.Q,
                           MW, NN, NO, n_controls, n_patients);
        FCD_LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(group_centre_kernel, gc, dim3(64 * GC_WAVES), 0, st, b, bt, C, (int)H, (int)U, KS, a.g.ws.XT, a.g.ws.Q);
        FCD_LAUNCH_CHECK();
        if (n_controls || n_patients) {
            hipLaunchKernelGGL(group_fill_counts_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, C, H, U, n_controls, n_patients);
            FCD_LAUNCH_CHECK();
        }
    }
    // the observed labelling: one packed row through the same tile product and the same t^2, each connection once
    a.g.P = 1;
    hipLaunchKernelGGL(group_pack_kernel, dim3((unsigned)((nw * 64 + 255) / 256)), dim3(256), 0, st, (const uint8_t *)nullptr, (int64_t)1,
                       (int)H, (int)S, nw, a.g.ws.LW);
    FCD_LAUNCH_CHECK();
    GPO_DISPATCH(group_observed_opt_kernel, flags, dim3((unsigned)((C + 16 * GP_WAVES - 1) / (16 * GP_WAVES))), dim3(64 * GP_WAVES), 0, st, a);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(group_observed_region_kernel, dim3((unsigned)N), dim3(64), 0, st, a.g.ws.t2obs, (int)N, region);
    FCD_LAUNCH_CHECK();
    a.g.P = P;
    const int64_t PG = (P + 15) / 16;
    hipLaunchKernelGGL(group_pack_kernel, dim3((unsigned)((PG * nw * 64 + 255) / 256)), dim3(256), 0, st, labels, P, (int)H, (int)S, nw,
                       a.g.ws.LW);
    FCD_LAUNCH_CHECK();
    GPO_DISPATCH(baseline_group_opt_kernel, flags, dim3((unsigned)N, (unsigned)gy), dim3(64 * GP_WAVES), 0, st, a);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(group_fold_kernel, dim3((unsigned)(N + (P + 255) / 256)), dim3(256), 0, st, a.g.ws.Rpart, a.g.ws.Mpart, region, (int)N, P,
                       null_max_region, null_max_t, count_region);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_baseline_network_bits_opt(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                             const uint8_t *labels, int64_t P, double threshold, int tail, int flags, uint32_t *bits,
                                             double *t, fcd_stream stream) {
    const char *who = "fcd_baseline_network_bits_opt";
    if (!ctx || !b || !bt || !bits) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    int rc = gpo_check(ctx, who, C, H, U, P, flags);
    if (rc) return rc;
    if (!flags) return fcd_baseline_network_bits(ctx, b, bt, C, H, U, labels, P, threshold, tail, bits, t, stream);
    if (!labels && P != 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "the observed labelling (labels == NULL) is P = 1, not %lld", P);
    if (!(threshold > 0.0) || !(threshold <= 1.7976931348623157e308))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "the threshold must be finite and > 0");
    if (tail < FCD_TAIL_BOTH || tail > FCD_TAIL_LESS) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "unknown tail %lld", tail);
    const int64_t S = H + U, N = fcd_C_to_N(C);
    if (N > NB_NMAX) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "%lld regions, at most %lld", N, NB_NMAX);
    const int64_t PG = (P + 15) / 16, gy = (PG + NBO_G - 1) / NBO_G, W = (C + 31) / 32;
    if (gy > 65535) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "shape too large (Nreg=%lld, P=%lld)", N, P);
    const int KS = (int)((S + 3) / 4), nw = (KS + 31) / 32;
    hipStream_t st = (hipStream_t)stream;
    // Nothing of the workspace outlives the call.
    const size_t base = nb_ws_bytes(C, P, KS, nw);
    rc = fcd_ws_reserve(ctx, base + gpo_conn_bytes(C, nw));
    if (rc) return rc;
    double *XT = (double *)ctx->ws, *Q = XT + (int64_t)KS * C * 4;
    uint32_t *LW = (uint32_t *)(Q + C), *MW = (uint32_t *)((char *)ctx->ws + base);
    int32_t *NN = (int32_t *)(MW + (int64_t)nw * C * 4), *NO = NN + C;
    const dim3 gc((unsigned)((C + GC_WAVES - 1) / GC_WAVES));
    if (flags & FCD_BASELINE_MISSING)
        hipLaunchKernelGGL(group_centre_missing_kernel, gc, dim3(64 * GC_WAVES), 0, st, b, bt, C, (int)H, (int)U, KS, nw, XT, Q, MW, NN, NO,
                           (int64_t *)nullptr, (int64_t *)nullptr);
    else
        hipLaunchKernelGGL(group_centre_kernel, gc, dim3(64 * GC_WAVES), 0, st, b, bt, C, (int)H, (int)U, KS, XT, Q);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(group_pack_kernel, dim3((unsigned)((PG * nw * 64 + 255) / 256)), dim3(256), 0, st, labels, P, (int)H, (int)S, nw, LW);
    FCD_LAUNCH_CHECK();
    nbo_args a;
    a.b.XT = XT;
    a.b.Q = Q;
    a.b.LW = LW;
    a.b.C = C;
    a.b.P = P;
    a.b.W2 = 2 * W;
    a.b.KS = KS;
    a.b.nw = nw;
    a.b.tail = tail;
    a.b.kf = 0.0;
    a.b.dof = 0.0;
    a.b.thr2 = threshold * threshold;
    a.b.bits = reinterpret_cast<uint16_t *>(bits);
    a.b.t = t;
    a.k.MW = MW;
    a.k.NN = NN;
    a.k.NO = NO;
    a.k.nS = (double)S;
    a.k.nU = (double)U;
    GPO_DISPATCH(network_bits_opt_kernel, flags, dim3((unsigned)((2 * W + GP_WAVES - 1) / GP_WAVES), (unsigned)gy), dim3(64 * GP_WAVES), 0, st, a);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_graph_components(fcd_ctx *ctx, const uint32_t *bits, int64_t B, int64_t C, int32_t *component, int32_t *n_edges,
                                    int32_t *max_extent, int32_t *max_regions, fcd_stream stream) {
    if (!ctx || !bits || !n_edges || !max_extent || !max_regions) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_graph_components: null pointer");
    if (B < 1 || C < 1) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_graph_components: B=%lld and C=%lld must be >= 1", B, C);
    const int64_t N = fcd_C_to_N(C);
    if (N < 2) return fcd_fail(ctx, FCD_ERR_SHAPE, "fcd_graph_components: C=%lld is not a triangular number", C);
    if (N > NB_NMAX) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_graph_components: %lld regions, at most %lld", N, NB_NMAX);
    if (B > INT32_MAX) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_graph_components: shape too large (Nreg=%lld, B=%lld)", N, B);
    const int64_t W = (C + 31) / 32;
    const size_t shmem = (size_t)(W + 3 * N + 4) * sizeof(uint32_t);
    int rc = fcd_lds_attr(ctx, FCD_KA_COMPONENTS, (const void *)graph_components_kernel, shmem);
    if (rc) return rc;
    hipLaunchKernelGGL(graph_components_kernel, dim3((unsigned)B), dim3(CC_T), shmem, (hipStream_t)stream, bits, C, (int)N, (int)W, component,
                       n_edges, max_extent, max_regions);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_baseline_group_glm(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                      const double *design, int64_t R, const uint16_t *perms, int64_t P, double *t, double *region,
                                      double *null_max_t, double *null_max_region, int64_t *count_t, int64_t *count_region,
                                      fcd_stream stream) {
    const char *who = "fcd_baseline_group_glm";
    if (!ctx || !b || !bt || !design || !perms || !t || !region || !null_max_t || !null_max_region || !count_t || !count_region)
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    int rc = glm_check(ctx, who, C, H, U, R, P);
    if (rc) return rc;
    const int64_t S = H + U, N = fcd_C_to_N(C);
    const int64_t gy = (P + GP_WAVES * GL_G * 16 - 1) / (GP_WAVES * GL_G * 16);
    if (N > 46340 || gy > 65535 || (C + GC_WAVES - 1) / GC_WAVES > INT32_MAX || N * P > (1ll << 34))
        return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "shape too large (Nreg=%lld, P=%lld)", N, P);
    const int KS4 = (int)((S + 15) / 16), KS = 4 * KS4;      // K-steps in whole quads: one index word each
    const int64_t PG = (P + 15) / 16;
    hipStream_t st = (hipStream_t)stream;
    // Nothing of the workspace outlives the call.  gp_ws without label words | index words (PG, KS4, 64) uint64
    const size_t base = gp_ws_bytes(C, N, P, KS, 0);
    rc = fcd_ws_reserve(ctx, base + (size_t)(PG * KS4 * 64) * sizeof(uint64_t));
    if (rc) return rc;
    glm_args a;
    a.ws = gp_ws_at(ctx->ws, C, N, P, KS);
    uint64_t *PI = (uint64_t *)((char *)ctx->ws + base);
    a.PI = PI;
    a.design = design;
    a.C = C;
    a.N = (int)N;
    a.KS = KS;
    a.S = (int)S;
    a.R = (int)R;
    a.dof = (double)(S - R - 1);
    a.t = t;
    a.count_t = reinterpret_cast<unsigned long long *>(count_t);
    FCD_HIP_TRY(hipMemsetAsync(count_t, 0, (size_t)C * sizeof(int64_t), st));
    hipLaunchKernelGGL(glm_centre_kernel, dim3((unsigned)((C + GC_WAVES - 1) / GC_WAVES)), dim3(64 * GC_WAVES),
                       (size_t)((R - 1) * S) * sizeof(double), st, b, bt, C, (int)H, (int)U, KS, design, (int)R, glm_dead2(S, R), a.ws.XT,
                       a.ws.Q);
    FCD_LAUNCH_CHECK();
    // the observed statistics: the identity as one packed row through the same tile product and the same t^2, each connection once
    a.P = 1;
    hipLaunchKernelGGL(glm_pack_kernel, dim3((unsigned)((KS4 * 64 + 255) / 256)), dim3(256), 0, st, (const uint16_t *)nullptr, (int64_t)1,
                       (int)S, KS4, PI);
    FCD_LAUNCH_CHECK();
    GLM_LAUNCH(glm_observed_kernel, 0, dim3((unsigned)((C + 16 * GP_WAVES - 1) / (16 * GP_WAVES))), st, a);
    hipLaunchKernelGGL(group_observed_region_kernel, dim3((unsigned)N), dim3(64), 0, st, a.ws.t2obs, (int)N, region);
    FCD_LAUNCH_CHECK();
    a.P = P;
    hipLaunchKernelGGL(glm_pack_kernel, dim3((unsigned)((PG * KS4 * 64 + 255) / 256)), dim3(256), 0, st, perms, P, (int)S, KS4, PI);
    FCD_LAUNCH_CHECK();
    GLM_LAUNCH(glm_group_kernel, 1, dim3((unsigned)N, (unsigned)gy), st, a);
    hipLaunchKernelGGL(group_fold_kernel, dim3((unsigned)(N + (P + 255) / 256)), dim3(256), 0, st, a.ws.Rpart, a.ws.Mpart, region, (int)N, P,
                       null_max_region, null_max_t, count_region);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_baseline_network_bits_glm(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                             const double *design, int64_t R, const uint16_t *perms, int64_t P, double threshold,
                                             int tail, uint32_t *bits, double *t, fcd_stream stream) {
    const char *who = "fcd_baseline_network_bits_glm";
    if (!ctx || !b || !bt || !design || !bits) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    int rc = glm_check(ctx, who, C, H, U, R, P);
    if (rc) return rc;
    if (!perms && P != 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "the identity (perms == NULL) is P = 1, not %lld", P);
    if (!(threshold > 0.0) || !(threshold <= 1.7976931348623157e308))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "the threshold must be finite and > 0");
    if (tail < FCD_TAIL_BOTH || tail > FCD_TAIL_LESS) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "unknown tail %lld", tail);
    const int64_t S = H + U, N = fcd_C_to_N(C);
    if (N > NB_NMAX) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "%lld regions, at most %lld", N, NB_NMAX);
    const int64_t PG = (P + 15) / 16, gy = (PG + GL_G - 1) / GL_G, W = (C + 31) / 32;
    if (gy > 65535) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "shape too large (Nreg=%lld, P=%lld)", N, P);
    const int KS4 = (int)((S + 15) / 16), KS = 4 * KS4;      // K-steps in whole quads: one index word each
    hipStream_t st = (hipStream_t)stream;
    // Nothing of the workspace outlives the call.  XT (KS, C, 4) | Q (C) | index words (PG, KS4, 64) uint64
    rc = fcd_ws_reserve(ctx, (size_t)((int64_t)KS * C * 4 + C) * sizeof(double) + (size_t)(PG * KS4 * 64) * sizeof(uint64_t));
    if (rc) return rc;
    double *XT = (double *)ctx->ws, *Q = XT + (int64_t)KS * C * 4;
    uint64_t *PI = (uint64_t *)(Q + C);
    hipLaunchKernelGGL(glm_centre_kernel, dim3((unsigned)((C + GC_WAVES - 1) / GC_WAVES)), dim3(64 * GC_WAVES),
                       (size_t)((R - 1) * S) * sizeof(double), st, b, bt, C, (int)H, (int)U, KS, design, (int)R, glm_dead2(S, R), XT, Q);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(glm_pack_kernel, dim3((unsigned)((PG * KS4 * 64 + 255) / 256)), dim3(256), 0, st, perms, P, (int)S, KS4, PI);
    FCD_LAUNCH_CHECK();
    glm_bits_args a;
    a.XT = XT;
    a.Q = Q;
    a.design = design;
    a.PI = PI;
    a.C = C;
    a.P = P;
    a.W2 = 2 * W;
    a.KS = KS;
    a.S = (int)S;
    a.R = (int)R;
    a.tail = tail;
    a.dof = (double)(S - R - 1);
    a.thr2 = threshold * threshold;
    a.bits = reinterpret_cast<uint16_t *>(bits);
    a.t = t;
    GLM_LAUNCH(glm_bits_kernel, 2, dim3((unsigned)((2 * W + GP_WAVES - 1) / GP_WAVES), (unsigned)gy), st, a);
    return FCD_OK;
}
