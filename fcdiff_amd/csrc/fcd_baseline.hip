// K_base: the classical baselines (fcd_baseline_normative, fcd_baseline_group_perm and fcd_baseline_network_bits with their _opt
// and _glm forms, fcd_baseline_network_excess, fcd_graph_components and its _weighted form).  Not in the reference; oracles =
// tests/baseline_ref.py, baseline_missing_ref.py, baseline_glm_ref.py, network_ref.py, network_intensity_ref.py.  E(n) = the N - 1 connections that touch region n, walked as k = 0 .. N - 2 with the
// other endpoint m = k (k < n) or k + 1: rows tri(n) + k are contiguous for k < n, rows tri(m) + n are strided for k >= n.  A
// connection is met by both its endpoints; what is written once per connection (z, z0, n_controls, count_t) is written by the
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
// Permutation tests: the group test (t per connection, sum of t^2 per region, the permutation law of the maxima) and the
// network-based statistic (t thresholded to one bit per labelling and connection, then graph_components_kernel).  Statistics in
// their t^2 form: one division per value, the root only where a t leaves the device.  Both are built from
//   a centre kernel    one wave per row of X = [b | bt]: what the statistic takes off the row, Q = the sum of squares of what is
//                      left, written K-step major: XT[j][c][0..3] = subjects 4 j .. 4 j + 3 of row c, zeros behind S.
//   a pack kernel      the rows of 16 labellings as the words a lane feeds the MFMA as its A operand, one group of 16 after
//                      the other; rows == nullptr: the observed labelling as the only row.
//   a statistic        (one of three, below): the tile product of 16 labellings x 16 connections over all K-steps in ascending
//                      order -- per K-step ONE 8-byte load per lane (lane l: row of connection l & 15, subject 4 j + (l >> 4);
//                      512 contiguous bytes where the 16 rows are contiguous, 32-byte pieces where they are strided: the same
//                      address formula), one v_mfma_f64_16x16x4_f64 per accumulator -- and the t^2 of a result element.
//   three shells       group_observed_kernel, group_perm_kernel, network_bits_kernel: templates over the statistic, which own
//                      the walk, the order of every addition, the masks, the counts and the stores.  Each rule below is stated
//                      at the shell that implements it, once for all three statistics.
//   group_observed_region_kernel, group_fold_kernel   the region sums of the observed t^2 and the fold of the (n, p) partials.
//
// The statistics (struct stat_*: what a wave keeps per group of 16 labellings, the tile product, liveness, t^2 and its sign)
//   stat_plain         pooled t on complete data.  A operand = a label bit expanded to 0.0 / 1.0 in two VALU instructions, the
//                      label words of a group (at most 8) in registers.  gp_t2: g = A^2 S/(U H), t^2 = g (S - 2) / (Q - g).
//                      Dead = constant: all S values equal (min == max, K_cov's rule; the centre kernel compares every value
//                      it reads with the first), centred values and Q exactly 0.  No value is ever undefined.
//   stat_opt<MISS, WELCH>   missing data and Welch's t; oracle = tests/baseline_missing_ref.py.  Never instantiated with both
//                      off: that is stat_plain, which has no division per value beside the one of t^2.  The label words again,
//                      and up to three accumulators through the same product: A = L X (XT holds 0 at a missing subject),
//                      n1 = L M (MISS; M the 0/1 observation mask, exact small integers in any order) and B = L X^2 (WELCH; the
//                      square of the value already loaded).  The mask takes the label words' treatment: MW[(w C + c) 4 + ks],
//                      bit j = subject 4 (32 w + j) + ks of row c is observed, one uint32 per lane and 32 K-steps.
//                      Defined: pooled Q > 0, n >= 3, n1 >= 1, n0 >= 1; Welch Q > 0, n1 >= 2, n0 >= 2.  Dead = undefined under
//                      the observed labelling; a value can be undefined under one labelling alone.
//   stat_glm<RT>       nuisance covariates, the permutation GLM of Freedman & Lane; oracle = tests/baseline_glm_ref.py.  The
//                      design W (S, R) is orthonormal, every column orthogonal to the constant; column 0 is tested given the
//                      others.  Per connection e = the residuals of the row on [1, w_1 .. w_{R-1}], Q_e = sum e^2; per
//                      permutation pi, d_q = sum_s W[pi[s], q] e_s, t^2 = d_0^2 dof / (Q_e - sum_q d_q^2), dof = S - R - 1, the
//                      sign of t that of d_0.  A operand = a double read from W in the workgroup's LDS ((S + 1, RT) rows, RT =
//                      2, 3, 5 or 9 >= R, zero columns behind R, a row of zeros behind S) by a permuted index: per group one
//                      8-byte index load per four K-steps, per MFMA one 8-byte LDS read at the lane's own row; the B value is
//                      loaded once per K-step and feeds all RT MFMAs of every group.  The observed statistics are those of
//                      the identity.  Dead: constant rows, and those with Q_e <= dead2 Q_c, dead2 = (8 S R 2^-52)^2: a linear
//                      function of the covariates to rounding (derivation: DESIGN.md).  No value is ever undefined.
//   Separated          (every statistic) the denominator of t^2, a difference of rounded numbers, not > 0 with Q > 0: t^2 = +inf,
//                      t = +/-inf with the sign of the numerator; inf >= inf counts.  No other finite input gives a NaN, and no
//                      region sum ever sees a negative term.
//
// Network-based statistic
//   graph_components_kernel  one workgroup per row of bits, the row in LDS (64 KB at 1024 regions, the limit).  label[x] = x;
//                      per round every set bit (n, m) pulls the larger label, and the region that label names, down to the
//                      smaller (LDS atomicMin), then label[x] = label[label[x]]; until a round changes nothing, at most N
//                      rounds.  Then extents, regions, maxima with integer LDS atomics.
//   component intensity  (fcd_baseline_network_excess, fcd_graph_components_weighted; oracle = tests/network_intensity_ref.py)
//                      network_bits_kernel<Stat, true> also stores max(|t| - threshold, 0) where a bit is set, and only there;
//                      graph_components_weighted_kernel sums those values per component in a fixed order.
#include "fcd_common.h"

#include <type_traits>

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int BN_WAVES = 4;
constexpr int BN_HMAX = 1024;            // controls of the normative kernel: one LDS row per wave
constexpr int GP_WAVES = 4;              // waves per workgroup of the three shells
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

// ---- permutation tests: centre and pack kernels ----------------------------------------------------------------------------

constexpr int GC_WAVES = 4;
constexpr int GL_RMAX = 9;               // design columns

// stat_plain, and stat_opt without MISS: the row minus its mean over the S subjects
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

// stat_opt with MISS: the mean over the observed subjects, 0 at a missing one; beside XT and Q the mask words, n = the observed
// subjects and the observed patients of every connection
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

// stat_glm: group_centre_kernel with the residualisation: columns 1 .. R - 1 of W in LDS (column-major), the mean, the R - 1
// coefficients a_q = sum w_q (x - mean) as wave sums, q ascending, then e = (x - mean) - sum_q w_q a_q (q ascending), Q_e and
// Q_c = sum (x - mean)^2.  Writes XT exactly as group_centre_kernel does.  A dead row has e and Q exactly 0.
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

// The labels of 16 labellings x 128 subjects as one uint32 per lane: bit j of lane l = label of labelling l & 15 at subject
// 4 (32 w + j) + (l >> 4) -- what that lane feeds the MFMA as A at K-step 32 w + j.  labels == nullptr: the observed labelling
// (ones on the last U subjects).
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

// The indices of 16 permutations x 4 K-steps as four uint16 in one uint64 per lane: field i of lane l of quad j4 =
// perms[16 pg + (l & 15)][4 (4 j4 + i) + (l >> 4)], what that lane feeds the MFMA as the row of W at K-step 4 j4 + i.  S -- the
// row of zeros behind W in LDS -- behind the last subject, behind the last permutation and for an index that is out of range.
// perms == nullptr: the identity.
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

// ---- tile products and t^2: where the statistics really differ --------------------------------------------------------------

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
// t^2 = NaN.  Two compares and two selects per value.
__device__ __forceinline__ double gp_t2(double A, double Qc, double kf, double dof) {
    const double gq = A * A * kf, den = Qc - gq;
    double t2 = gq * dof / den;
    if (!(den > 0.0)) t2 = __builtin_inf();
    if (!(Qc > 0.0)) t2 = __builtin_nan("");
    return t2;
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

// the design's rows in the workgroup's dynamic LDS
__device__ __forceinline__ double *glm_lds() {
    extern __shared__ double gl_w[];
    return gl_w;
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
// ascending order; KS is a multiple of 4 here (the centre kernel writes zeros behind S, the pack kernel the zero row).  xp as in
// gp_tile_mma; ip[g]: this lane's index word of quad 0 of group g, 64 words to the next quad.
template <int RT, int G>
__device__ __forceinline__ void glm_tile_mma(const double *__restrict__ xp, int64_t jstride, const uint64_t *const (&ip)[G],
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

// ---- the three statistics: what the shells ask of one ------------------------------------------------------------------------
//   args               its kernel arguments, behind the shell's own
//   GP_G, NB_G         groups of 16 labellings per wave of the permutation pass and of the bits pass (the grids follow)
//   prologue           by the whole workgroup, before any wave returns
//   state<G>, load     what a wave keeps for its G groups, read once
//   tile<G>, product   the tile product of the G groups at connection c, and the per-connection values it needs
//   live               (permutation pass) is the connection live under the observed labelling, whose t^2 is t2o?
//   alive              (bits pass) the same from the connection's own values: no second pass
//   t2                 t^2 of result element r of group g, its sign-carrying numerator, whether it is defined
//   lds_bytes, lds_slot   (host) its dynamic LDS, and the fcd_lds_attr slot of shell `which` = 0, 1, 2, 3

struct plain_args {
    const uint32_t *LW;
    int nw;
    double kf, dof;                    // S / (U H), S - 2
};
// per connection, beside XT and Q: mask words, n = observed subjects, n1 of the observed labelling (observed patients)
struct gpo_conn {
    const uint32_t *MW;
    const int32_t *NN, *NO;
    double nS, nU;                     // what n and n1 are on complete data (MISS off)
};
struct opt_args {
    const uint32_t *LW;
    int nw;
    gpo_conn k;
};
struct glm_args {
    const uint64_t *PI;
    const double *design;
    int S, R;
    double dof;                        // S - R - 1
};

template <int G>
struct lw_state {
    uint32_t lw[G][GP_NW];
};
template <int G>
struct gp_tile_t {
    double4_t acc[G];
    double Qc;
};
template <int G>
struct gpo_tile_t {
    double4_t acc[G], accn[G], accb[G];
    double Qc, nc;
    bool counted;
};
template <int G>
struct glm_state {
    const uint64_t *ip[G];
};
template <int RT, int G>
struct glm_tile_t {
    double4_t acc[G][RT];
    double Qc;
};

__host__ static inline int glm_width(int R) { return R <= 2 ? 0 : R <= 3 ? 1 : R <= 5 ? 2 : 3; }      // RT = 2, 3, 5, 9

// stat_plain and stat_opt: the label words of a wave's groups in registers (at most G x 8); no LDS, no barrier
struct stat_labels {
    template <int G>
    using state = lw_state<G>;
    template <class A>
    static __device__ __forceinline__ void prologue(const A &) {}
    template <int G, class A>
    static __device__ __forceinline__ void load(lw_state<G> &w, const A &s, int, int64_t pg0, int64_t PG, int lane) {
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int x = 0; x < GP_NW; ++x) w.lw[g][x] = (x < s.nw && pg0 + g < PG) ? s.LW[((pg0 + g) * s.nw + x) * 64 + lane] : 0u;
    }
    template <class A>
    static size_t lds_bytes(const A &) { return 0; }
    static int lds_slot(int) { return 0; }
};

struct stat_plain : stat_labels {
    typedef plain_args args;
    static constexpr int GP_G = 2, NB_G = 4;
    template <int G>
    using tile = gp_tile_t<G>;
    template <int G>
    static __device__ __forceinline__ void product(gp_tile_t<G> &x, const lw_state<G> &w, const args &s, const double *__restrict__ XT,
                                                   const double *__restrict__ Q, int64_t C, int64_t c, int ks, int KS) {
        gp_tile_mma<G>(XT + c * 4 + ks, C * 4, w.lw, s.nw, KS, x.acc);
        x.Qc = Q[c];
    }
    template <int G>
    static __device__ __forceinline__ bool live(const gp_tile_t<G> &x, double) { return x.Qc > 0.0; }
    template <int G>
    static __device__ __forceinline__ bool alive(const gp_tile_t<G> &, const args &, int64_t) { return true; }   // (NaN compares false)
    template <int G>
    static __device__ __forceinline__ double t2(const gp_tile_t<G> &x, const args &s, int g, int r, double &num, bool &def) {
        num = x.acc[g][r];
        def = true;
        return gp_t2(num, x.Qc, s.kf, s.dof);
    }
};

template <bool MISS, bool WELCH>
struct stat_opt : stat_labels {
    typedef opt_args args;
    static constexpr int GP_G = 2, NB_G = 2;                 // (three accumulators per group)
    template <int G>
    using tile = gpo_tile_t<G>;
    template <int G>
    static __device__ __forceinline__ void product(gpo_tile_t<G> &x, const lw_state<G> &w, const args &s, const double *__restrict__ XT,
                                                   const double *__restrict__ Q, int64_t C, int64_t c, int ks, int KS) {
        const double *__restrict__ xp = XT + c * 4 + ks;
        const uint32_t *__restrict__ mp = MISS ? s.k.MW + c * 4 + ks : nullptr;
        x.nc = MISS ? (double)s.k.NN[c] : s.k.nS;
        if (G == 1) {                                        // the observed pass: no shortcut (8 VGPRs for one MFMA in three, once)
            gpo_tile_mma<G, MISS, WELCH>(xp, C * 4, mp, C * 4, w.lw, s.nw, KS, x.acc, x.accn, x.accb);
            x.counted = MISS;
        } else {
            x.counted = gpo_tile<G, MISS, WELCH>(xp, C * 4, mp, C * 4, w.lw, s.nw, KS, x.nc, s.k.nS, x.acc, x.accn, x.accb);
        }
        x.Qc = Q[c];
    }
    template <int G>
    static __device__ __forceinline__ bool live(const gpo_tile_t<G> &, double t2o) { return t2o == t2o; }
    template <int G>
    static __device__ __forceinline__ bool alive(const gpo_tile_t<G> &x, const args &s, int64_t c) {
        bool def;
        (void)gpo_t2<WELCH>(0.0, 0.0, MISS ? (double)s.k.NO[c] : s.k.nU, x.nc, x.Qc, def);
        return def;
    }
    template <int G>
    static __device__ __forceinline__ double t2(const gpo_tile_t<G> &x, const args &s, int g, int r, double &num, bool &def) {
        num = x.acc[g][r];
        return gpo_t2<WELCH>(num, x.accb[g][r], x.counted ? x.accn[g][r] : s.k.nU, x.nc, x.Qc, def);
    }
};

template <int RT>
struct stat_glm {
    typedef glm_args args;
    static constexpr int GP_G = 2, NB_G = 2;                 // (G * RT accumulators of 8 VGPRs)
    template <int G>
    using state = glm_state<G>;
    template <int G>
    using tile = glm_tile_t<RT, G>;
    static __device__ __forceinline__ void prologue(const args &s) { glm_load_design<RT>(s.design, s.S, s.R, glm_lds()); }
    template <int G>
    static __device__ __forceinline__ void load(glm_state<G> &w, const args &s, int KS, int64_t pg0, int64_t PG, int lane) {
#pragma unroll
        for (int g = 0; g < G; ++g) w.ip[g] = s.PI + (pg0 + g < PG ? pg0 + g : PG - 1) * (KS >> 2) * 64 + lane;   // (behind the last: masked)
    }
    template <int G>
    static __device__ __forceinline__ void product(glm_tile_t<RT, G> &x, const glm_state<G> &w, const args &, const double *__restrict__ XT,
                                                   const double *__restrict__ Q, int64_t C, int64_t c, int ks, int KS) {
        glm_tile_mma<RT, G>(XT + c * 4 + ks, C * 4, w.ip, glm_lds(), KS, x.acc);
        x.Qc = Q[c];
    }
    template <int G>
    static __device__ __forceinline__ bool live(const glm_tile_t<RT, G> &x, double) { return x.Qc > 0.0; }
    template <int G>
    static __device__ __forceinline__ bool alive(const glm_tile_t<RT, G> &, const args &, int64_t) { return true; }   // (NaN compares false)
    template <int G>
    static __device__ __forceinline__ double t2(const glm_tile_t<RT, G> &x, const args &s, int g, int r, double &num, bool &def) {
        num = x.acc[g][0][r];
        def = true;
        return glm_t2<RT>(x.acc[g], r, x.Qc, s.dof);
    }
    static size_t lds_bytes(const args &s) { return (size_t)(s.S + 1) * RT * sizeof(double); }
    static int lds_slot(int which) { return FCD_KA_GLM + 4 * which + glm_width(RT); }
};

// ---- the three shells --------------------------------------------------------------------------------------------------------
// In all three a wave's tile is 16 connections (lane & 15 = column) x G groups of 16 labellings; result element r of group g in
// lane l belongs to labelling (pg0 + g) 16 + (l >> 4) + 4 r.  A column past the last connection reads the last row and is
// masked.  Each returns wave by wave once the statistic's prologue is done: no workgroup barrier behind it.

struct gp_common {
    const double *XT, *Q;
    double *t2obs, *Rpart, *Mpart;
    int64_t C, P;
    int N, KS;
    double *t;                         // the observed shell's
    unsigned long long *count_t;       // the permutation shell's
};
template <class A>
struct gp_kargs {
    gp_common c;
    A s;
};

// The observed labelling (the one row the pack kernel made of it): a wave per 16 consecutive connections, each connection
// once.  Row 0 of the tile is the labelling: lanes 0 .. 15, result element 0.  Writes t and t^2, NaN where the connection is dead.
template <class Stat>
__global__ __launch_bounds__(64 * GP_WAVES) void group_observed_kernel(gp_kargs<typename Stat::args> a) {
    Stat::prologue(a.s);
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t C = a.c.C, c0 = ((int64_t)blockIdx.x * GP_WAVES + wv) * 16;
    if (c0 >= C) return;                                     // (no workgroup barrier below)
    const int col = lane & 15, ks = lane >> 4;
    const int64_t c = c0 + col < C ? c0 + col : C - 1;
    typename Stat::template state<1> w;
    Stat::load(w, a.s, a.c.KS, 0, 1, lane);
    typename Stat::template tile<1> x;
    Stat::product(x, w, a.s, a.c.XT, a.c.Q, C, c, ks, a.c.KS);
    if (ks == 0 && c0 + col < C) {
        double num;
        bool def;
        double t2 = Stat::t2(x, a.s, 0, 0, num, def);
        if (!def) t2 = __builtin_nan("");
        a.c.t2obs[c] = t2;
        a.c.t[c] = copysign(sqrt(t2), num);
    }
}

// ... and its region sums.  THE ADDITION ORDER of a region sum, here and in the permutation shell: lane = column of the tile, a
// running sum over the tiles in tile order, then the butterfly over the 16 columns.  A row equal to the observed labelling (the
// identity) therefore gives the observed statistics bit for bit: the same operations on the same numbers in the same order.
// A dead connection (t^2 = NaN) adds exactly 0.
__global__ __launch_bounds__(64) void group_observed_region_kernel(const double *__restrict__ t2obs, int N, double *__restrict__ region) {
    const int n = blockIdx.x, col = threadIdx.x & 15;
    double rs = 0.0;
    for (int k0 = 0; k0 < N - 1; k0 += 16) {
        const int k = k0 + col;
        const bool valid = k < N - 1;
        int m;
        double t2 = t2obs[bl_edge(n, valid ? k : N - 2, m)];
        if (!valid || t2 != t2) t2 = 0.0;
        rs += t2;
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) rs += __shfl_xor(rs, o, 64);
    if (threadIdx.x == 0) region[n] = rs;
}

// The permutation pass: grid (N, blocks of 64 G labellings), 4 waves x G groups.  A wave reads its state once, then walks E(n)
// in tiles of 16 connections.  Per lane a running sum and maximum of t^2 over the tiles (tile order), folded over the 16 lanes
// of a labelling by the fixed butterfly after the last tile: the (n, p) partials.
//   dead connection    (not live under the observed labelling) exactly 0 to the sums, no maximum, no count.
//   undefined value    (under this labelling alone) 0 to the sums and no maximum, but an exceedance: a labelling that cannot
//                      be evaluated never makes a p-value smaller.
//   count_t            t^2 >= the observed t^2, counted by the endpoint n > m: one integer atomic per tile and connection.
template <class Stat>
__global__ __launch_bounds__(64 * GP_WAVES) void group_perm_kernel(gp_kargs<typename Stat::args> a) {
    constexpr int G = Stat::GP_G;
    Stat::prologue(a.s);
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = blockIdx.x, N = a.c.N;
    const int64_t C = a.c.C, P = a.c.P, PG = (P + 15) / 16;
    const int64_t pg0 = ((int64_t)blockIdx.y * GP_WAVES + wv) * G;
    if (pg0 >= PG) return;                                   // (no workgroup barrier below)
    const int col = lane & 15, ks = lane >> 4;
    typename Stat::template state<G> w;
    Stat::load(w, a.s, a.c.KS, pg0, PG, lane);
    double rs[G][4], mx[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) rs[g][r] = mx[g][r] = 0.0;
    for (int k0 = 0; k0 < N - 1; k0 += 16) {
        const int k = k0 + col;
        const bool valid = k < N - 1;
        int m;
        const int64_t c = bl_edge(n, valid ? k : N - 2, m);
        typename Stat::template tile<G> x;
        Stat::product(x, w, a.s, a.c.XT, a.c.Q, C, c, ks, a.c.KS);
        const double t2o = a.c.t2obs[c];
        const bool live = valid && Stat::live(x, t2o);
        const bool own = live && k < n;
        int cnt = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double num;
                bool def;
                double t2 = Stat::t2(x, a.s, g, r, num, def);
                if (!live || !def) t2 = 0.0;                 // (own implies live: a defined value is compared as it stands)
                const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
                cnt += (own && p < P && (!def || t2 >= t2o)) ? 1 : 0;
                rs[g][r] += t2;
                mx[g][r] = fmax(mx[g][r], t2);
            }
        }
        cnt += __shfl_xor(cnt, 16, 64);
        cnt += __shfl_xor(cnt, 32, 64);
        if (own && ks == 0 && cnt) atomicAdd(&a.c.count_t[c], (unsigned long long)cnt);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
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
                a.c.Rpart[(int64_t)n * P + p] = s;
                a.c.Mpart[(int64_t)n * P + p] = v;
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

constexpr int NB_NMAX = 1024;            // regions of the components kernel: a row of bits lives in LDS (64 KB at 1024)
constexpr int CC_T = 256;                // its threads

struct nb_common {
    const double *XT, *Q;
    int64_t C, P, W2;                  // W2 = 2 W: the 16-bit pieces of a row of bits
    int KS, tail;
    double thr2;
    uint16_t *bits;
    double *t;                         // nullable: the t of labelling 0
};
template <class A>
struct nb_kargs {
    nb_common c;
    A s;
};
// what the excess form takes on top: nb_kargs stays the argument of the plain form, byte for byte
template <class A>
struct nb_xargs : nb_kargs<A> {
    double *excess;                    // (P, 32 W): written only where the bit is set
    double thr;
};

// The bits pass: each connection once (half of the permutation pass's matrix work), nothing kept but one bit per (labelling,
// connection).  A wave: 16 consecutive connections (piece blockIdx.x * 4 + wave of a row of bits) x G groups of labellings.
// The ballot of a compare holds, in its 16-bit field ks, the 16 connections of labelling (pg0 + g) 16 + ks + 4 r: shifted by
// 16 ks, lane 16 ks stores it (plain vector stores).  A piece behind the last connection (C <= 32 W - 16) is written as zeros.
// No bit for a dead connection under any labelling, none for an undefined value; t of labelling 0 is NaN at either.  The
// observed labelling is a call with P = 1.
// X, the excess form: behind the ballot a lane whose own bit is set takes the root and stores max(|t| - threshold, 0) at
// excess[p 32 W + c] (plain vector stores; 16 lanes of a labelling write 128 contiguous bytes).  Nothing is stored, and no
// root taken, for an unset bit; the product, t^2 and the compare are the plain form's, so its bits are.
template <class Stat, bool X = false>
__global__ __launch_bounds__(64 * GP_WAVES) void network_bits_kernel(
    typename std::conditional<X, nb_xargs<typename Stat::args>, nb_kargs<typename Stat::args>>::type a) {
    constexpr int G = Stat::NB_G;
    Stat::prologue(a.s);
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t piece = (int64_t)blockIdx.x * GP_WAVES + wv;
    if (piece >= a.c.W2) return;                             // (no workgroup barrier below)
    const int64_t C = a.c.C, P = a.c.P, PG = (P + 15) / 16, c0 = piece * 16;
    const int64_t pg0 = (int64_t)blockIdx.y * G;
    const int col = lane & 15, ks = lane >> 4;
    if (c0 >= C) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
                if (col == 0 && p < P) a.c.bits[p * a.c.W2 + piece] = (uint16_t)0;
            }
        }
        return;
    }
    const bool valid = c0 + col < C;
    const int64_t c = valid ? c0 + col : C - 1;
    typename Stat::template state<G> w;
    Stat::load(w, a.s, a.c.KS, pg0, PG, lane);
    typename Stat::template tile<G> x;
    Stat::product(x, w, a.s, a.c.XT, a.c.Q, C, c, ks, a.c.KS);
    const bool alive = Stat::alive(x, a.s, c);
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double num;
            bool def;
            const double t2 = Stat::t2(x, a.s, g, r, num, def);
            const bool side = a.c.tail == 0 || (a.c.tail == 1 ? num > 0.0 : num < 0.0);
            const bool set = valid && alive && def && side && t2 > a.c.thr2;
            const unsigned long long mask = __ballot(set);
            const int64_t p = (pg0 + g) * 16 + ks + 4 * r;
            if (col == 0 && p < P) a.c.bits[p * a.c.W2 + piece] = (uint16_t)(mask >> (16 * ks));
            if constexpr (X) {
                if (set && p < P) a.excess[p * (16 * a.c.W2) + c] = fmax(sqrt(t2) - a.thr, 0.0);
            }
            if (a.c.t && p == 0 && valid) a.c.t[c] = (alive && def) ? copysign(sqrt(t2), num) : __builtin_nan("");
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

struct ccw_args {
    const uint32_t *bits;
    const double *weights;             // (B, 32 W): read only where the bit is set
    int64_t C;
    int N, W;
    int32_t *component, *n_edges, *max_extent, *max_regions;
    double *intensity, *max_intensity;
};

// The same with a weight per set bit.  LDS as above, then (8-byte aligned) s[N] doubles and the maximum as one 64-bit word.
// Labels, extents and regions exactly as graph_components_kernel makes them; then, with no floating-point atomic:
//   s[n]               one thread per region: the weights of the set bits of row n (connections tri(n) .. tri(n) + n - 1, each
//                      connection in the row of its larger endpoint), added in ascending connection order;
//   a component's sum  one thread per root: s[y] over its regions y in ascending order (y >= the root, its smallest region);
//   the maximum        weights are >= 0, so the sums order as their bit patterns do: a 64-bit integer atomicMax.
// Every sum is a fixed sequence of additions of this row's values alone: the same bits whatever B or the row's place.
__global__ __launch_bounds__(CC_T) void graph_components_weighted_kernel(ccw_args a) {
    extern __shared__ uint32_t cc_lds[];
    const int N = a.N, W = a.W;
    uint32_t *words = cc_lds;
    int *label = (int *)(words + W), *extent = label + N, *regions = extent + N, *sc = regions + N;
    double *s = (double *)(cc_lds + ((W + 3 * N + 4 + 1) & ~1));
    unsigned long long *smax = (unsigned long long *)(s + N);
    const int tid = threadIdx.x;
    const uint32_t *__restrict__ src = a.bits + (int64_t)blockIdx.x * W;
    const double *__restrict__ wt = a.weights + (int64_t)blockIdx.x * W * 32;
    const uint32_t last = (a.C & 31) ? (1u << (a.C & 31)) - 1u : ~0u;      // bits behind C are ignored
    for (int w = tid; w < W; w += CC_T) words[w] = src[w] & (w == W - 1 ? last : ~0u);
    for (int x = tid; x < N; x += CC_T) {
        label[x] = x;
        extent[x] = 0;
        regions[x] = 0;
    }
    if (tid < 4) sc[tid] = 0;
    if (tid == 0) *smax = 0ull;
    __syncthreads();
    for (int round = 0; round < N; ++round) {                // the fixed point of graph_components_kernel
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
        for (int x = tid; x < N; x += CC_T) {
            const int l = label[x], ll = label[l];
            if (ll < l) atomicMin(&label[x], ll);
        }
        __syncthreads();
        if (!changed) break;
        if (tid == 0) sc[0] = 0;
        __syncthreads();
    }
    for (int w = tid; w < W; w += CC_T) cc_for_bits(w, words[w], [&](int n, int) { atomicAdd(&extent[label[n]], 1); });
    for (int n = tid; n < N; n += CC_T) {                    // row sums: word by word, set bits in ascending order
        double sum = 0.0;
        const int c0 = (int)fcd_tri(n), c1 = c0 + n;         // (n = 0: no row)
        for (int w = c0 >> 5; w <= (c1 - 1) >> 5 && c1 > c0; ++w) {
            uint32_t word = words[w];
            if (w == c0 >> 5) word &= ~0u << (c0 & 31);
            if (w == c1 >> 5) word &= (1u << (c1 & 31)) - 1u;
            while (word) {
                const int j = __ffs((int)word) - 1;
                word &= word - 1u;
                sum += wt[w * 32 + j];
            }
        }
        s[n] = sum;
    }
    __syncthreads();
    for (int x = tid; x < N; x += CC_T) {
        const int l = label[x];
        if (extent[l] > 0) atomicAdd(&regions[l], 1);
    }
    __syncthreads();
    for (int x = tid; x < N; x += CC_T) {
        const int e = extent[x], l = label[x];
        double total = 0.0;
        if (e > 0) {                                         // x is a root
            atomicAdd(&sc[1], e);
            atomicMax(&sc[2], e);
            atomicMax(&sc[3], regions[x]);
            for (int y = x; y < N; ++y)
                if (label[y] == x) total += s[y];
            atomicMax(smax, (unsigned long long)__double_as_longlong(total));
        }
        if (a.component) a.component[(int64_t)blockIdx.x * N + x] = extent[l] > 0 ? l : -1;
        if (a.intensity) a.intensity[(int64_t)blockIdx.x * N + x] = total;
    }
    __syncthreads();
    if (tid == 0) {
        a.n_edges[blockIdx.x] = sc[1];
        a.max_extent[blockIdx.x] = sc[2];
        a.max_regions[blockIdx.x] = sc[3];
        a.max_intensity[blockIdx.x] = __longlong_as_double((long long)*smax);
    }
}

// ---- host: checks, the statistics' host sides, the two sequences -----------------------------------------------------------

struct bl_in {                         // what every permutation call is given
    const double *b, *bt;
    int64_t C, H, U, P;
};

// what all six calls check alike; who = the call's name, null = one of its required pointers is
__host__ static int bl_check(fcd_ctx *ctx, const char *who, bool null, const bl_in &d) {
    if (null) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    if (d.C < 1 || d.H < 1 || d.U < 1 || d.P < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "C, H, U=%lld and P=%lld must be >= 1", d.U, d.P);
    if (fcd_C_to_N(d.C) < 2) return fcd_fail_who(ctx, FCD_ERR_SHAPE, who, "C=%lld is not a triangular number", d.C);
    if (d.H + d.U > GP_SMAX) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "%lld subjects, at most %lld", d.H + d.U, GP_SMAX);
    return FCD_OK;
}

// what the three bits calls check alike; no_rows: the refusal of rows == NULL at P != 1, in the call's own words
__host__ static int nb_check(fcd_ctx *ctx, const char *who, const bl_in &d, bool rows, const char *no_rows, double threshold, int tail) {
    if (!rows && d.P != 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, no_rows, d.P);
    if (!(threshold > 0.0) || !(threshold <= 1.7976931348623157e308))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "the threshold must be finite and > 0");
    if (tail < FCD_TAIL_BOTH || tail > FCD_TAIL_LESS) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "unknown tail %lld", tail);
    if (fcd_C_to_N(d.C) > NB_NMAX) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "%lld regions, at most %lld", fcd_C_to_N(d.C), NB_NMAX);
    return FCD_OK;
}

// each statistic's own
__host__ static int plain_check(fcd_ctx *ctx, const char *who, const bl_in &d) {
    if (d.H + d.U < 3) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "%lld subjects, a pooled variance needs 3", d.H + d.U);
    return FCD_OK;
}
__host__ static int opt_check(fcd_ctx *ctx, const char *who, const bl_in &d, int flags) {
    if (flags & ~(FCD_BASELINE_MISSING | FCD_BASELINE_WELCH)) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "unknown flags 0x%llx", flags);
    int rc = plain_check(ctx, who, d);
    if (rc) return rc;
    if ((flags & FCD_BASELINE_WELCH) && (d.H < 2 || d.U < 2))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "welch: H=%lld and U=%lld must be >= 2, a variance per group", d.H, d.U);
    return FCD_OK;
}
__host__ static int glm_check(fcd_ctx *ctx, const char *who, const bl_in &d, int64_t R) {
    if (R < 1 || R > GL_RMAX) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "R=%lld design columns, 1 to %lld", R, GL_RMAX);
    if (d.H + d.U < R + 2) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "%lld subjects, R=%lld design columns need R + 2", d.H + d.U, R);
    return FCD_OK;
}

// one shell of one statistic; which = 0, 1, 2, 3: observed, permutations, bits, bits with excess
template <class Stat, class A>
__host__ static int bl_launch(fcd_ctx *ctx, void (*kern)(A), int which, dim3 grid, hipStream_t st, A &a) {
    const size_t shmem = Stat::lds_bytes(a.s);
    int rc = fcd_lds_attr(ctx, Stat::lds_slot(which), reinterpret_cast<const void *>(kern), shmem);    // (raises the limit past 64 KB)
    if (rc) return rc;
    void *args[] = {&a};
    FCD_HIP_TRY(hipLaunchKernel(reinterpret_cast<const void *>(kern), grid, dim3(64 * GP_WAVES), args, shmem, st));
    return FCD_OK;
}

// The host side of a statistic:
//   any                one of its instances: they share args and the groups per wave
//   ks                 K-steps of S subjects
//   bytes              what it appends to a pass's workspace
//   setup              carves that part at `own`, fills its kernel arguments, launches its centre kernel
//   pack               its pack kernel: the observed row, or the call's rows
//   pick               calls f with the instance the call's options select

__host__ static inline int64_t lw_words(const bl_in &d, int nw) { return (d.P + 15) / 16 * nw * 64; }
__host__ static int lw_pack(hipStream_t st, const bl_in &d, const uint8_t *rows, int64_t P, int nw, const uint32_t *LW) {
    hipLaunchKernelGGL(group_pack_kernel, dim3((unsigned)(((P + 15) / 16 * nw * 64 + 255) / 256)), dim3(256), 0, st, rows, P, (int)d.H,
                       (int)(d.H + d.U), nw, const_cast<uint32_t *>(LW));
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
__host__ static inline dim3 gc_grid(int64_t C) { return dim3((unsigned)((C + GC_WAVES - 1) / GC_WAVES)); }

struct plain_host {
    typedef stat_plain any;
    const uint8_t *labels;
    static int ks(int64_t S) { return (int)((S + 3) / 4); }
    size_t bytes(const bl_in &d, int KS) const { return (size_t)lw_words(d, (KS + 31) / 32) * sizeof(uint32_t); }
    int setup(fcd_ctx *, hipStream_t st, const bl_in &d, int KS, double *XT, double *Q, void *own, plain_args &s) const {
        s.LW = (const uint32_t *)own;
        s.nw = (KS + 31) / 32;
        s.kf = (double)(d.H + d.U) / ((double)d.U * (double)d.H);
        s.dof = (double)(d.H + d.U - 2);
        hipLaunchKernelGGL(group_centre_kernel, gc_grid(d.C), dim3(64 * GC_WAVES), 0, st, d.b, d.bt, d.C, (int)d.H, (int)d.U, KS, XT, Q);
        FCD_LAUNCH_CHECK();
        return FCD_OK;
    }
    int pack(hipStream_t st, const bl_in &d, int, const plain_args &s, bool observed) const {
        return lw_pack(st, d, observed ? nullptr : labels, observed ? 1 : d.P, s.nw, s.LW);
    }
    template <class F>
    int pick(F f) const { return f(stat_plain()); }
};

struct opt_host {
    typedef stat_opt<true, true> any;
    const uint8_t *labels;
    int flags;                         // FCD_BASELINE_MISSING, FCD_BASELINE_WELCH: not 0
    int64_t *n_controls, *n_patients;  // nullable
    static int ks(int64_t S) { return (int)((S + 3) / 4); }
    // label words | MW (nw, C, 4) uint32 | NN (C) int32 | NO (C) int32
    size_t bytes(const bl_in &d, int KS) const {
        const int nw = (KS + 31) / 32;
        return (size_t)(lw_words(d, nw) + (int64_t)nw * d.C * 4 + 2 * d.C) * sizeof(uint32_t);
    }
    int setup(fcd_ctx *, hipStream_t st, const bl_in &d, int KS, double *XT, double *Q, void *own, opt_args &s) const {
        const int nw = (KS + 31) / 32;
        uint32_t *MW = (uint32_t *)own + lw_words(d, nw);
        int32_t *NN = (int32_t *)(MW + (int64_t)nw * d.C * 4), *NO = NN + d.C;
        s.LW = (const uint32_t *)own;
        s.nw = nw;
        s.k.MW = MW;
        s.k.NN = NN;
        s.k.NO = NO;
        s.k.nS = (double)(d.H + d.U);
        s.k.nU = (double)d.U;
        if (flags & FCD_BASELINE_MISSING) {
            hipLaunchKernelGGL(group_centre_missing_kernel, gc_grid(d.C), dim3(64 * GC_WAVES), 0, st, d.b, d.bt, d.C, (int)d.H, (int)d.U, KS, nw,
                               XT, Q, MW, NN, NO, n_controls, n_patients);
            FCD_LAUNCH_CHECK();
            return FCD_OK;
        }
        hipLaunchKernelGGL(group_centre_kernel, gc_grid(d.C), dim3(64 * GC_WAVES), 0, st, d.b, d.bt, d.C, (int)d.H, (int)d.U, KS, XT, Q);
        FCD_LAUNCH_CHECK();
        if (n_controls || n_patients) {
            hipLaunchKernelGGL(group_fill_counts_kernel, dim3((unsigned)((d.C + 255) / 256)), dim3(256), 0, st, d.C, d.H, d.U, n_controls,
                               n_patients);
            FCD_LAUNCH_CHECK();
        }
        return FCD_OK;
    }
    int pack(hipStream_t st, const bl_in &d, int, const opt_args &s, bool observed) const {
        return lw_pack(st, d, observed ? nullptr : labels, observed ? 1 : d.P, s.nw, s.LW);
    }
    template <class F>
    int pick(F f) const {
        if (flags == FCD_BASELINE_MISSING) return f(stat_opt<true, false>());
        if (flags == FCD_BASELINE_WELCH) return f(stat_opt<false, true>());
        return f(stat_opt<true, true>());
    }
};

struct glm_host {
    typedef stat_glm<2> any;
    const double *design;
    int R;
    const uint16_t *perms;
    static int ks(int64_t S) { return 4 * (int)((S + 15) / 16); }      // K-steps in whole quads: one index word each
    // index words (PG, KS / 4, 64) uint64
    size_t bytes(const bl_in &d, int KS) const { return (size_t)((d.P + 15) / 16 * (KS >> 2) * 64) * sizeof(uint64_t); }
    int setup(fcd_ctx *, hipStream_t st, const bl_in &d, int KS, double *XT, double *Q, void *own, glm_args &s) const {
        const int64_t S = d.H + d.U;
        const double tol = 8.0 * (double)S * (double)R * 2.220446049250313e-16;
        s.PI = (const uint64_t *)own;
        s.design = design;
        s.S = (int)S;
        s.R = R;
        s.dof = (double)(S - R - 1);
        hipLaunchKernelGGL(glm_centre_kernel, gc_grid(d.C), dim3(64 * GC_WAVES), (size_t)((R - 1) * S) * sizeof(double), st, d.b, d.bt, d.C,
                           (int)d.H, (int)d.U, KS, design, R, tol * tol, XT, Q);
        FCD_LAUNCH_CHECK();
        return FCD_OK;
    }
    int pack(hipStream_t st, const bl_in &d, int KS, const glm_args &s, bool observed) const {
        const int64_t P = observed ? 1 : d.P;
        hipLaunchKernelGGL(glm_pack_kernel, dim3((unsigned)(((P + 15) / 16 * (KS >> 2) * 64 + 255) / 256)), dim3(256), 0, st,
                           observed ? nullptr : perms, P, s.S, KS >> 2, const_cast<uint64_t *>(s.PI));
        FCD_LAUNCH_CHECK();
        return FCD_OK;
    }
    template <class F>
    int pick(F f) const {
        switch (glm_width(R)) {
        case 0: return f(stat_glm<2>());
        case 1: return f(stat_glm<3>());
        case 2: return f(stat_glm<5>());
        default: return f(stat_glm<9>());
        }
    }
};

struct gp_out {
    double *t, *region, *null_max_t, *null_max_region;
    int64_t *count_t, *count_region;
};

// The group test.  Workspace: XT (KS, C, 4) | Q (C) | t2obs (C) | Rpart (N, P) | Mpart (N, P) | the statistic's; nothing of it
// outlives the call.  The observed labelling goes as one packed row through the same tile product and the same t^2.
template <class Host>
__host__ static int gp_run(fcd_ctx *ctx, const char *who, const bl_in &d, const Host &h, const gp_out &o, hipStream_t st) {
    typedef typename Host::any::args A;
    constexpr int PB = GP_WAVES * Host::any::GP_G * 16;      // labellings per workgroup
    const int64_t C = d.C, P = d.P, N = fcd_C_to_N(C), gy = (P + PB - 1) / PB;
    if (N > 46340 || gy > 65535 || (C + GC_WAVES - 1) / GC_WAVES > INT32_MAX || N * P > (1ll << 34))
        return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "shape too large (Nreg=%lld, P=%lld)", N, P);
    const int KS = Host::ks(d.H + d.U);
    const size_t base = (size_t)((int64_t)KS * C * 4 + 2 * C + 2 * N * P) * sizeof(double);
    int rc = fcd_ws_reserve(ctx, base + h.bytes(d, KS));
    if (rc) return rc;
    double *XT = (double *)ctx->ws.p, *Q = XT + (int64_t)KS * C * 4;
    gp_kargs<A> a;
    a.c.XT = XT;
    a.c.Q = Q;
    a.c.t2obs = Q + C;
    a.c.Rpart = a.c.t2obs + C;
    a.c.Mpart = a.c.Rpart + N * P;
    a.c.C = C;
    a.c.P = P;
    a.c.N = (int)N;
    a.c.KS = KS;
    a.c.t = o.t;
    a.c.count_t = reinterpret_cast<unsigned long long *>(o.count_t);
    FCD_HIP_TRY(hipMemsetAsync(o.count_t, 0, (size_t)C * sizeof(int64_t), st));
    if ((rc = h.setup(ctx, st, d, KS, XT, Q, (char *)ctx->ws.p + base, a.s))) return rc;
    if ((rc = h.pack(st, d, KS, a.s, true))) return rc;
    rc = h.pick([&](auto s) {
        typedef decltype(s) Stat;
        return bl_launch<Stat>(ctx, group_observed_kernel<Stat>, 0, dim3((unsigned)((C + 16 * GP_WAVES - 1) / (16 * GP_WAVES))), st, a);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(group_observed_region_kernel, dim3((unsigned)N), dim3(64), 0, st, a.c.t2obs, (int)N, o.region);
    FCD_LAUNCH_CHECK();
    if ((rc = h.pack(st, d, KS, a.s, false))) return rc;
    rc = h.pick([&](auto s) {
        typedef decltype(s) Stat;
        return bl_launch<Stat>(ctx, group_perm_kernel<Stat>, 1, dim3((unsigned)N, (unsigned)gy), st, a);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(group_fold_kernel, dim3((unsigned)(N + (P + 255) / 256)), dim3(256), 0, st, a.c.Rpart, a.c.Mpart, o.region, (int)N, P,
                       o.null_max_region, o.null_max_t, o.count_region);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

// The bits of P labellings (rows == NULL: of the observed one).  Workspace: XT (KS, C, 4) | Q (C) | the statistic's.
// excess != nullptr: the excess form of the kernel, which also writes the excess of every set bit.
template <class Host>
__host__ static int nb_run(fcd_ctx *ctx, const char *who, const bl_in &d, const Host &h, double threshold, int tail, uint32_t *bits,
                           double *t, hipStream_t st, double *excess = nullptr) {
    typedef typename Host::any::args A;
    constexpr int PB = Host::any::NB_G * 16;                 // labellings per wave
    const int64_t C = d.C, P = d.P, gy = (P + PB - 1) / PB, W = (C + 31) / 32;
    if (gy > 65535) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "shape too large (Nreg=%lld, P=%lld)", fcd_C_to_N(C), P);
    const int KS = Host::ks(d.H + d.U);
    const size_t base = (size_t)((int64_t)KS * C * 4 + C) * sizeof(double);
    int rc = fcd_ws_reserve(ctx, base + h.bytes(d, KS));
    if (rc) return rc;
    double *XT = (double *)ctx->ws.p, *Q = XT + (int64_t)KS * C * 4;
    nb_xargs<A> a;
    a.excess = excess;
    a.thr = threshold;
    a.c.XT = XT;
    a.c.Q = Q;
    a.c.C = C;
    a.c.P = P;
    a.c.W2 = 2 * W;
    a.c.KS = KS;
    a.c.tail = tail;
    a.c.thr2 = threshold * threshold;
    a.c.bits = reinterpret_cast<uint16_t *>(bits);
    a.c.t = t;
    if ((rc = h.setup(ctx, st, d, KS, XT, Q, (char *)ctx->ws.p + base, a.s))) return rc;
    if ((rc = h.pack(st, d, KS, a.s, false))) return rc;
    const dim3 grid((unsigned)((2 * W + GP_WAVES - 1) / GP_WAVES), (unsigned)gy);
    return h.pick([&](auto s) {
        typedef decltype(s) Stat;
        if (excess) return bl_launch<Stat>(ctx, network_bits_kernel<Stat, true>, 3, grid, st, a);
        return bl_launch<Stat>(ctx, network_bits_kernel<Stat>, 2, grid, st, static_cast<nb_kargs<A> &>(a));
    });
}

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
    const char *who = "fcd_baseline_group_perm";
    const bl_in d = {b, bt, C, H, U, P};
    int rc = bl_check(ctx, who, !ctx || !b || !bt || !labels || !t || !region || !null_max_t || !null_max_region || !count_t || !count_region, d);
    if (!rc) rc = plain_check(ctx, who, d);
    if (rc) return rc;
    return gp_run(ctx, who, d, plain_host{labels}, gp_out{t, region, null_max_t, null_max_region, count_t, count_region}, (hipStream_t)stream);
}

extern "C" int fcd_baseline_network_bits(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                         const uint8_t *labels, int64_t P, double threshold, int tail, uint32_t *bits, double *t,
                                         fcd_stream stream) {
    const char *who = "fcd_baseline_network_bits";
    const bl_in d = {b, bt, C, H, U, P};
    int rc = bl_check(ctx, who, !ctx || !b || !bt || !bits, d);
    if (!rc) rc = plain_check(ctx, who, d);
    if (!rc) rc = nb_check(ctx, who, d, labels, "the observed labelling (labels == NULL) is P = 1, not %lld", threshold, tail);
    if (rc) return rc;
    return nb_run(ctx, who, d, plain_host{labels}, threshold, tail, bits, t, (hipStream_t)stream);
}

extern "C" int fcd_baseline_group_perm_opt(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                           const uint8_t *labels, int64_t P, int flags, double *t, double *region, double *null_max_t,
                                           double *null_max_region, int64_t *count_t, int64_t *count_region, int64_t *n_controls,
                                           int64_t *n_patients, fcd_stream stream) {
    const char *who = "fcd_baseline_group_perm_opt";
    const bl_in d = {b, bt, C, H, U, P};
    int rc = bl_check(ctx, who, !ctx || !b || !bt || !labels || !t || !region || !null_max_t || !null_max_region || !count_t || !count_region, d);
    if (!rc) rc = opt_check(ctx, who, d, flags);
    if (rc) return rc;
    if (!flags) {                                            // no option: the call without them, and the counts it implies
        rc = fcd_baseline_group_perm(ctx, b, bt, C, H, U, labels, P, t, region, null_max_t, null_max_region, count_t, count_region, stream);
        if (rc || (!n_controls && !n_patients)) return rc;
        hipLaunchKernelGGL(group_fill_counts_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, C, H, U, n_controls,
                           n_patients);
        FCD_LAUNCH_CHECK();
        return FCD_OK;
    }
    return gp_run(ctx, who, d, opt_host{labels, flags, n_controls, n_patients},
                  gp_out{t, region, null_max_t, null_max_region, count_t, count_region}, (hipStream_t)stream);
}

extern "C" int fcd_baseline_network_bits_opt(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                             const uint8_t *labels, int64_t P, double threshold, int tail, int flags, uint32_t *bits,
                                             double *t, fcd_stream stream) {
    const char *who = "fcd_baseline_network_bits_opt";
    const bl_in d = {b, bt, C, H, U, P};
    int rc = bl_check(ctx, who, !ctx || !b || !bt || !bits, d);
    if (!rc) rc = opt_check(ctx, who, d, flags);
    if (rc) return rc;
    if (!flags) return fcd_baseline_network_bits(ctx, b, bt, C, H, U, labels, P, threshold, tail, bits, t, stream);
    rc = nb_check(ctx, who, d, labels, "the observed labelling (labels == NULL) is P = 1, not %lld", threshold, tail);
    if (rc) return rc;
    return nb_run(ctx, who, d, opt_host{labels, flags, nullptr, nullptr}, threshold, tail, bits, t, (hipStream_t)stream);
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
    const bl_in d = {b, bt, C, H, U, P};
    int rc = bl_check(ctx, who,
                      !ctx || !b || !bt || !design || !perms || !t || !region || !null_max_t || !null_max_region || !count_t || !count_region, d);
    if (!rc) rc = glm_check(ctx, who, d, R);
    if (rc) return rc;
    return gp_run(ctx, who, d, glm_host{design, (int)R, perms}, gp_out{t, region, null_max_t, null_max_region, count_t, count_region},
                  (hipStream_t)stream);
}

extern "C" int fcd_baseline_network_bits_glm(fcd_ctx *ctx, const double *b, const double *bt, int64_t C, int64_t H, int64_t U,
                                             const double *design, int64_t R, const uint16_t *perms, int64_t P, double threshold,
                                             int tail, uint32_t *bits, double *t, fcd_stream stream) {
    const char *who = "fcd_baseline_network_bits_glm";
    const bl_in d = {b, bt, C, H, U, P};
    int rc = bl_check(ctx, who, !ctx || !b || !bt || !design || !bits, d);
    if (!rc) rc = glm_check(ctx, who, d, R);
    if (!rc) rc = nb_check(ctx, who, d, perms, "the identity (perms == NULL) is P = 1, not %lld", threshold, tail);
    if (rc) return rc;
    return nb_run(ctx, who, d, glm_host{design, (int)R, perms}, threshold, tail, bits, t, (hipStream_t)stream);
}

extern "C" int fcd_baseline_network_excess(fcd_ctx *ctx, const fcd_network_excess_desc *x) {
    static const char *who = "fcd_baseline_network_excess";
    if (!ctx) return FCD_ERR_ARG;
    if (!x) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null descriptor");
    if (x->size != sizeof(fcd_network_excess_desc))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "descriptor size %lld, this library's is %lld", x->size,
                            (long long)sizeof(fcd_network_excess_desc));
    const bl_in d = {x->b, x->bt, x->C, x->H, x->U, x->P};
    const bool glm = x->design != nullptr;
    int rc = bl_check(ctx, who, !x->b || !x->bt || !x->bits || !x->excess, d);
    if (rc) return rc;
    if (glm && x->flags) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "flags 0x%llx with a design: the covariate form has no options", x->flags);
    rc = glm ? glm_check(ctx, who, d, x->R) : opt_check(ctx, who, d, (int)x->flags);
    if (!rc)
        rc = glm ? nb_check(ctx, who, d, x->perms, "the identity (perms == NULL) is P = 1, not %lld", x->threshold, x->tail)
                 : nb_check(ctx, who, d, x->labels, "the observed labelling (labels == NULL) is P = 1, not %lld", x->threshold, x->tail);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)x->stream;
    if (glm) return nb_run(ctx, who, d, glm_host{x->design, (int)x->R, x->perms}, x->threshold, x->tail, x->bits, x->t, st, x->excess);
    if (x->flags) return nb_run(ctx, who, d, opt_host{x->labels, (int)x->flags, nullptr, nullptr}, x->threshold, x->tail, x->bits, x->t, st, x->excess);
    return nb_run(ctx, who, d, plain_host{x->labels}, x->threshold, x->tail, x->bits, x->t, st, x->excess);
}

extern "C" int fcd_graph_components_weighted(fcd_ctx *ctx, const fcd_components_desc *x) {
    static const char *who = "fcd_graph_components_weighted";
    if (!ctx) return FCD_ERR_ARG;
    if (!x) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null descriptor");
    if (x->size != sizeof(fcd_components_desc))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "descriptor size %lld, this library's is %lld", x->size, (long long)sizeof(fcd_components_desc));
    if (x->flags) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "unknown flags 0x%llx", x->flags);
    if (!x->bits || !x->weights || !x->n_edges || !x->max_extent || !x->max_regions || !x->max_intensity)
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    if (x->B < 1 || x->C < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "B=%lld and C=%lld must be >= 1", x->B, x->C);
    const int64_t N = fcd_C_to_N(x->C);
    if (N < 2) return fcd_fail_who(ctx, FCD_ERR_SHAPE, who, "C=%lld is not a triangular number", x->C);
    if (N > NB_NMAX) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "%lld regions, at most %lld", N, NB_NMAX);
    if (x->B > INT32_MAX) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "shape too large (Nreg=%lld, B=%lld)", N, x->B);
    const int64_t W = (x->C + 31) / 32;
    const size_t shmem = (size_t)((W + 3 * N + 4 + 1) & ~(int64_t)1) * sizeof(uint32_t) + (size_t)(N + 1) * sizeof(double);
    int rc = fcd_lds_attr(ctx, FCD_KA_COMPONENTS_W, (const void *)graph_components_weighted_kernel, shmem);
    if (rc) return rc;
    ccw_args a = {x->bits,      x->weights,    x->C,           (int)N,       (int)W,          x->component,
                  x->n_edges,   x->max_extent, x->max_regions, x->intensity, x->max_intensity};
    hipLaunchKernelGGL(graph_components_weighted_kernel, dim3((unsigned)x->B), dim3(CC_T), shmem, (hipStream_t)x->stream, a);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
