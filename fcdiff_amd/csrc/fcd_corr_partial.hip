// K_partial: per-subject partial correlations with shrinkage towards the identity -> edge-major (C, S), the layout of K_corr.
//
// Not in the reference (its inputs are already correlations); oracle = tests/partial_corr_ref.py (numpy.longdouble).
// Per subject s, over its first n = n_frames[s] frames (include/fcdiff_hip.h has the rules in full):
//   R        sample correlation matrix of the live rows (a region is dead where K_corr gives NaN on all of its edges)
//   R_a      (1 - a) R + a I,  a given or Ledoit & Wolf (2004) on the standardised rows
//   Theta    R_a^-1 by blocked Gauss-Jordan without pivoting (R_a is symmetric positive definite with unit diagonal)
//   rho_ij   -Theta_ij / sqrt(Theta_ii Theta_jj)
// The correlations come from fcd_corr_edges' own kernels (fcd_corr_edges_at, fcd_corr.hip): no second Gram product here.
// Subjects are walked in chunks so that the dense matrices never exceed PC_MAT_BYTES; no sum crosses a subject, so the
// chunking changes no bit.  Every reduction has a fixed order; there are no floating-point atomics.
#include "fcd_common.h"

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int PNB = 16;                       // columns per step of the inversion: one MFMA tile
constexpr int PC_JC = 8;                      // column tiles per work item of the rank-16 update (one set of A fragments)
constexpr double PC_PIVOT_MIN = 1e-12;        // a pivot at or below this: the subject is numerically singular
constexpr size_t PC_MAT_BYTES = (size_t)256 << 20;
constexpr int PC_TB = 256;                    // frames per workgroup of the frame-norm kernel

// global stores of this wave have been acknowledged, then the barrier: the next phase of the SAME workgroup (same CU, same L1)
// reads what this one wrote
__device__ __forceinline__ void pc_sync() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

__device__ __forceinline__ double pc_readlane(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// items of the update in the tile rows before I: row i has i / PC_JC + 1 of them
__host__ __device__ constexpr int pc_items_before(int I) {
    return I + PC_JC * ((I / PC_JC) * (I / PC_JC - 1) / 2) + (I % PC_JC) * (I / PC_JC);
}
constexpr int PC_ITEMS_MAX = pc_items_before(1024 / PNB);

__device__ __forceinline__ int pc_frames(const int32_t *n_frames, int64_t s, int T) { return n_frames ? n_frames[s] : T; }

// redge (C, Sc), subjects fastest -> the two triangles of A (Sc, PL, PL).  32 edges x 32 subjects through LDS: the loads are
// coalesced along s, the stores of the lower triangle along m (consecutive edges of a row are consecutive columns).
__global__ __launch_bounds__(256) void pc_dense_kernel(const double *__restrict__ redge, int64_t Sc, int64_t C, int PL,
                                                       double *__restrict__ A) {
    __shared__ double tile[32][33];
    const int64_t c0 = (int64_t)blockIdx.x * 32, s0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int64_t c = c0 + ty + j, s = s0 + tx;
        if (s < Sc && c < C) tile[ty + j][tx] = redge[c * Sc + s];
    }
    __syncthreads();
    const int64_t c = c0 + tx;
    if (c >= C) return;
    int n, m;
    fcd_edge_to_pair(c, n, m);
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int64_t s = s0 + ty + j;
        if (s >= Sc) continue;
        const double v = tile[tx][ty + j];
        double *M = A + s * PL * PL;
        M[(int64_t)n * PL + m] = v;
        M[(int64_t)m * PL + n] = v;
    }
}

// A wave per (subject, row): the row's live flag (a finite edge somewhere in it) and the sum of its squared finite
// off-diagonals, lanes along the row, the wave's fixed tree.
__global__ __launch_bounds__(256) void pc_rows_kernel(const double *__restrict__ A, int Nreg, int PL, int32_t *__restrict__ live,
                                                      double *__restrict__ rowF) {
    const int64_t s = blockIdx.y;
    const int l = threadIdx.x & 63, i = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= PL) return;
    const double *row = A + (s * PL + i) * PL;
    double q = 0.0;
    int any = 0;
    if (i < Nreg) {
        for (int j = l; j < Nreg; j += 64) {
            if (j == i) continue;
            const double v = row[j];
            if (v == v) {
                any = 1;
                q += v * v;
            }
        }
    }
    q = fcd_wave_sum(q);
    any = __any(any) ? 1 : 0;
    if (l == 0) {
        rowF[s * PL + i] = q;
        live[s * PL + i] = any;
    }
}

// A wave per subject: p_live, F = p + the rows' sums (lane l adds rows l, l + 64, ... in order, then the wave's tree) and the
// first status (2: fewer than two live regions, 3: n_frames outside [0, T]).
__global__ __launch_bounds__(64) void pc_total_kernel(const int32_t *__restrict__ live, const double *__restrict__ rowF, int PL, int T,
                                                      const int32_t *__restrict__ n_frames, int64_t s_base,
                                                      double *__restrict__ Fsum, int32_t *__restrict__ info) {
    const int64_t s = blockIdx.x;
    const int l = threadIdx.x;
    double f = 0.0;
    int p = 0;
    for (int i = l; i < PL; i += 64) {
        f += rowF[s * PL + i];
        p += live[s * PL + i];
    }
    f = fcd_wave_sum(f);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
    if (l == 0) {
        const int n = pc_frames(n_frames, s_base + s, T);
        Fsum[s] = (double)p + f;
        info[(s_base + s) * 2] = p;
        info[(s_base + s) * 2 + 1] = (n < 0 || n > T) ? 3 : (p < 2 ? 2 : 0);
    }
}

// Ledoit-Wolf only.  Mean and 1 / s_i of every live row over the subject's first n frames (s_i^2 = sum (x - m)^2 / n); a dead
// row gets 0, 0 and so drops out of the frame norms.  One wave per row.
__global__ __launch_bounds__(256) void pc_moments_kernel(const double *__restrict__ ts, int64_t rows, int Nreg, int PL, int T,
                                                         const int32_t *__restrict__ n_frames, int64_t s_base,
                                                         const int32_t *__restrict__ live, const int32_t *__restrict__ info,
                                                         double *__restrict__ mean, double *__restrict__ isd) {
    const int l = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t s = row / Nreg;
    const int i = (int)(row - s * Nreg);
    double mu = 0.0, is = 0.0;
    if (live[s * PL + i] && info[(s_base + s) * 2 + 1] == 0) {
        const int n = pc_frames(n_frames, s_base + s, T);
        const double *x = ts + row * T;
        double a = 0.0;
        for (int k = l; k < n; k += 64) a += x[k];
        a = fcd_wave_sum(a);
        mu = a / (double)n;
        double q = 0.0;
        for (int k = l; k < n; k += 64) {
            const double d = x[k] - mu;
            q += d * d;
        }
        q = fcd_wave_sum(q);
        const double var = q / (double)n;
        is = var > 0.0 ? 1.0 / sqrt(var) : 0.0;
    }
    if (l == 0) {
        mean[row] = mu;
        isd[row] = is;
    }
}

// Ledoit-Wolf only.  q_t = sum_i z_it^2 per (subject, frame): a thread per frame (coalesced along T), the regions in the
// loop; the workgroup's sum of q_t^2 over its PC_TB frames in a fixed tree -> qpart[s][block].
__global__ __launch_bounds__(PC_TB) void pc_frame_kernel(const double *__restrict__ ts, int Nreg, int T,
                                                         const int32_t *__restrict__ n_frames, int64_t s_base,
                                                         const double *__restrict__ mean, const double *__restrict__ isd,
                                                         int NBT, double *__restrict__ qpart) {
    __shared__ double sm[1024], si[1024], red[PC_TB / 64];
    const int64_t s = blockIdx.y;
    const int tid = threadIdx.x;
    for (int i = tid; i < Nreg; i += PC_TB) {
        sm[i] = mean[s * Nreg + i];
        si[i] = isd[s * Nreg + i];
    }
    __syncthreads();
    int n = pc_frames(n_frames, s_base + s, T);
    n = n < 0 ? 0 : (n > T ? T : n);
    const int t = (int)blockIdx.x * PC_TB + tid;
    double q = 0.0;
    if (t < n) {
        const double *x = ts + s * Nreg * T + t;
        for (int i = 0; i < Nreg; ++i) {
            if (si[i] == 0.0) continue;                 // (uniform over the workgroup)
            const double z = (x[(int64_t)i * T] - sm[i]) * si[i];
            q += z * z;
        }
    }
    double b = fcd_wave_sum(q * q);
    if ((tid & 63) == 0) red[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) {
        b = red[0];
        for (int k = 1; k < PC_TB / 64; ++k) b += red[k];
        qpart[s * NBT + blockIdx.x] = b;
    }
}

// alpha of the subject, and R_alpha in place over the raw copy: row i of the subject per workgroup.  Every workgroup makes
// alpha from the same numbers in the same order (B = the frame kernel's partial sums, in block order); row 0 reports it.
// A dead or padding row becomes an identity row, and so does every row of a subject whose status is set.
__global__ __launch_bounds__(256) void pc_shrink_kernel(double *__restrict__ A, int Nreg, int PL, int T,
                                                        const int32_t *__restrict__ n_frames, int64_t s_base,
                                                        const int32_t *__restrict__ live, const double *__restrict__ Fsum,
                                                        const double *__restrict__ qpart, int NBT, int shrink_mode,
                                                        double shrink_value, const int32_t *__restrict__ info,
                                                        double *__restrict__ alpha) {
    const int64_t s = blockIdx.y;
    const int i = blockIdx.x;
    const int status = info[(s_base + s) * 2 + 1];
    double a = shrink_value;
    if (status != 0) {
        a = __longlong_as_double(0x7ff8000000000000ll);
    } else if (shrink_mode == 1) {
        const double p = (double)info[(s_base + s) * 2], n = (double)pc_frames(n_frames, s_base + s, T);
        double B = 0.0;
        for (int k = 0; k < NBT; ++k) B += qpart[s * NBT + k];
        const double F = Fsum[s];
        const double beta = (B / n - F) / (p * n), delta = (F - p) / p;
        a = (delta > 0.0 && beta > 0.0) ? fmin(beta, delta) / delta : 0.0;
    }
    if (i == 0 && threadIdx.x == 0) alpha[s_base + s] = a;
    double *row = A + (s * PL + i) * PL;
    const bool li = status == 0 && i < Nreg && live[s * PL + i];
    const double om = 1.0 - a;
    for (int j = threadIdx.x; j < PL; j += 256) {
        double v;
        if (j == i) v = 1.0;
        else if (li && j < Nreg && live[s * PL + j]) v = om * row[j];
        else v = 0.0;
        row[j] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// The inversion: one workgroup per subject, the matrix (PL x PL, PL = 16 RT, identity beyond the live block) in global
// memory / the XCD's L2, inverted in place by blocked Gauss-Jordan in RT steps of 16 columns.  Step k:
//   1  wave 0 inverts the 16 x 16 pivot block A_kk in registers (unblocked Gauss-Jordan, the elements in the layout of an
//      MFMA result, rows and columns handed round with shuffles) -> P in LDS; a pivot <= PC_PIVOT_MIN marks the subject
//   2  row panel  W_J = P A_kJ  (J != k) -> LDS
//   3  rank-16 update  A_IJ -= A_Ik W_J  (I, J != k), v_mfma_f64_16x16x4_f64, the old column panel read from memory
//   4  column panel  A_Ik = -A_Ik P;  A_kJ = W_J;  A_kk = P
// Only the tiles I >= J are kept and updated: of the Gauss-Jordan state, A_IJ = -A_JI^T where exactly one of I, J has been
// a pivot block already and +A_JI^T otherwise, so every operand is a kept tile or the transpose of one (tests/
// partial_corr_ref.py restates the steps tile by tile).  p^3 flops and p / 16 passes over p^2 / 2 doubles, read and written.
// With one subject in flight per CU the matrices of a call do not fit the L2s (100 x 346 KB at 200 regions), so the passes
// go to memory: the kernel is bound by those bytes at 400 regions and by them and the chain of 4 RT barriers at 200, not by the
// matrix pipe.  Fragments as in fcd_corr.hip: A[i][k] in lane (i = l & 15, k = l >> 4), B[k][j] in lane (j = l & 15,
// k = l >> 4), D[i][j] as 4 doubles per lane, col = l & 15, row = (l >> 4) + 4 r.  A product over 16 columns is four MFMAs;
// the sum does not care which four columns go into which, so MFMA g takes columns 4 (l >> 4) + g from both operands: a
// lane's four A values are then 32 contiguous bytes of the column panel (two 16-byte loads).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void pc_invert_kernel(double *__restrict__ A, int PL, int RT, int WLD, int64_t s_base,
                                                         int32_t *__restrict__ info, double *__restrict__ dinv) {
    extern __shared__ __attribute__((aligned(16))) double psm[];
    double *W = psm, *P = psm + (size_t)PNB * WLD;      // W [16][WLD], P [16][17]
    __shared__ int sing;
    __shared__ short item_I[PC_ITEMS_MAX], item_J0[PC_ITEMS_MAX];
    const int64_t s = blockIdx.x;
    if (info[(s_base + s) * 2 + 1] != 0) return;         // (uniform) nothing to invert: the emit kernel writes NaN
    double *M = A + s * PL * PL;
    const int tid = threadIdx.x, l = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NW = (int)blockDim.x >> 6;
    const int i16 = l & 15, kq = l >> 4;
    // the items of the update, dealt round-robin to the waves: (tile row I, first tile column J0) for J0 = 0, PC_JC, ... <= I
    const int n_items = pc_items_before(RT);
    for (int I = tid; I < RT; I += (int)blockDim.x) {
        const int at = pc_items_before(I);
        for (int c = 0; c <= I / PC_JC; ++c) {
            item_I[at + c] = (short)I;
            item_J0[at + c] = (short)(c * PC_JC);
        }
    }
    if (tid == 0) sing = 0;
    __syncthreads();
    for (int k = 0; k < RT; ++k) {
        const int k0 = k * PNB;
        if (w == 0) {
            double a[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = M[(int64_t)(k0 + kq + 4 * r) * PL + k0 + i16];
            bool bad = false;
#pragma unroll
            for (int t = 0; t < PNB; ++t) {
                const int tr = t >> 2, tl = (t & 3) * 16;
                double piv = pc_readlane(a[tr], tl + t);                     // (a fixed lane: no trip through the LDS crossbar)
                if (!(piv > PC_PIVOT_MIN)) {
                    bad = true;
                    piv = 1.0;
                }
                const double d = 1.0 / piv;
                const double rowv = __shfl(a[tr], tl + i16, 64) * d;         // A[t][j] / pivot
                double colv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) colv[r] = __shfl(a[r], kq * 16 + t, 64);      // A[i][t], i = kq + 4 r
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = kq + 4 * r;
                    double v;
                    if (i == t) v = (i16 == t) ? d : rowv;
                    else if (i16 == t) v = -colv[r] * d;
                    else v = a[r] - colv[r] * rowv;
                    a[r] = v;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) P[(kq + 4 * r) * 17 + i16] = a[r];
            if (bad && l == 0) sing = 1;
        }
        __syncthreads();
        // 2: the row panel, from tile (k, J) where it is kept (J < k) and from the transpose of (J, k) where not
        for (int J = w; J < RT; J += NW) {
            if (J == k) continue;
            double fb[4];
            if (J < k) {
#pragma unroll
                for (int g = 0; g < 4; ++g) fb[g] = M[(int64_t)(k0 + kq * 4 + g) * PL + J * PNB + i16];
            } else {
                const double2 *bp = reinterpret_cast<const double2 *>(M + (int64_t)(J * PNB + i16) * PL + k0 + kq * 4);
                const double2 b01 = bp[0], b23 = bp[1];
                fb[0] = b01.x, fb[1] = b01.y, fb[2] = b23.x, fb[3] = b23.y;
            }
            double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int g = 0; g < 4; ++g) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(P[i16 * 17 + kq * 4 + g], fb[g], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) W[(kq + 4 * r) * WLD + J * PNB + i16] = acc[r];
        }
        __syncthreads();
        // 3: the update of the kept tiles outside row and column block k.  An item is up to PC_JC tiles of one tile row: all
        // their loads are asked for before the first MFMA and nothing is stored before the last (a store in between would
        // hold back the next tile's loads: the compiler cannot tell that they do not alias).  -A_Ik is minus tile (I, k)
        // below the pivot block and plus the transpose of tile (k, I) above it.
        for (int it = w; it < n_items; it += NW) {
            const int I = item_I[it], J0 = item_J0[it];
            if (I == k) continue;
            double fa[4];
            if (I > k) {
                const double2 *ap = reinterpret_cast<const double2 *>(M + (int64_t)(I * PNB + i16) * PL + k0 + kq * 4);
                const double2 a01 = ap[0], a23 = ap[1];
                fa[0] = -a01.x, fa[1] = -a01.y, fa[2] = -a23.x, fa[3] = -a23.y;
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) fa[g] = M[(int64_t)(k0 + kq * 4 + g) * PL + I * PNB + i16];
            }
            double *c0 = M + (int64_t)(I * PNB + kq) * PL + J0 * PNB + i16;
            double4_t acc[PC_JC];
#pragma unroll
            for (int u = 0; u < PC_JC; ++u) {
                acc[u] = double4_t{0.0, 0.0, 0.0, 0.0};
                if (J0 + u <= I && J0 + u != k) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[u][r] = c0[(int64_t)(4 * r) * PL + u * PNB];
                }
            }
#pragma unroll
            for (int u = 0; u < PC_JC; ++u) {
                if (J0 + u <= I && J0 + u != k) {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[g], W[(kq * 4 + g) * WLD + (J0 + u) * PNB + i16], acc[u], 0, 0, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < PC_JC; ++u) {
                if (J0 + u <= I && J0 + u != k) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) c0[(int64_t)(4 * r) * PL + u * PNB] = acc[u][r];
                }
            }
        }
        pc_sync();
        // 4: the column panel below the pivot block, the row panel left of it, and the pivot block, to memory
        for (int I = w; I < RT; I += NW) {
            if (I == k) {
#pragma unroll
                for (int r = 0; r < 4; ++r) M[(int64_t)(k0 + kq + 4 * r) * PL + k0 + i16] = P[(kq + 4 * r) * 17 + i16];
            } else if (I < k) {
#pragma unroll
                for (int r = 0; r < 4; ++r) M[(int64_t)(k0 + kq + 4 * r) * PL + I * PNB + i16] = W[(kq + 4 * r) * WLD + I * PNB + i16];
            } else {
                const double2 *ap = reinterpret_cast<const double2 *>(M + (int64_t)(I * PNB + i16) * PL + k0 + kq * 4);
                const double2 a01 = ap[0], a23 = ap[1];
                const double fa[4] = {-a01.x, -a01.y, -a23.x, -a23.y};
                double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int g = 0; g < 4; ++g) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[g], P[(kq * 4 + g) * 17 + i16], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) M[(int64_t)(I * PNB + kq + 4 * r) * PL + k0 + i16] = acc[r];
            }
        }
        pc_sync();
    }
    for (int i = tid; i < PL; i += (int)blockDim.x) dinv[s * PL + i] = 1.0 / sqrt(M[(int64_t)i * PL + i]);
    if (tid == 0 && sing) info[(s_base + s) * 2 + 1] = 1;
}

// rho from Theta back into edge-major (C, S): the reads run along m within a row of Theta, the stores along s.
__global__ __launch_bounds__(256) void pc_emit_kernel(const double *__restrict__ A, const double *__restrict__ dinv,
                                                      const int32_t *__restrict__ live, const int32_t *__restrict__ info,
                                                      int PL, int64_t Sc, int64_t s_base, int64_t S, int64_t C, int fisher_z,
                                                      double *__restrict__ out) {
    __shared__ double tile[32][33];
    const int64_t c0 = (int64_t)blockIdx.x * 32, s0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t c = c0 + tx;
    int n = 1, m = 0;
    if (c < C) fcd_edge_to_pair(c, n, m);
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int64_t s = s0 + ty + j;
        if (s >= Sc || c >= C) continue;
        double v = __longlong_as_double(0x7ff8000000000000ll);
        if (info[(s_base + s) * 2 + 1] == 0 && live[s * PL + n] && live[s * PL + m]) {
            v = -A[(s * PL + n) * PL + m] * dinv[s * PL + n] * dinv[s * PL + m];
            v = (v != v) ? v : fmin(fmax(v, -1.0), 1.0);
            if (fisher_z) v = atanh(v);
        }
        tile[ty + j][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int64_t cc = c0 + ty + j, s = s0 + tx;
        if (s < Sc && cc < C) out[cc * S + s_base + s] = tile[tx][ty + j];
    }
}

inline size_t pc_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

void fcd_corr_shrunk_plan(int64_t SC, int64_t Nreg, int64_t T, size_t base, fcd_shrunk_ws &w, bool with_A) {
    const int64_t C = fcd_tri(Nreg);
    w.RT = (int)((Nreg + PNB - 1) / PNB);
    w.PL = w.RT * PNB;
    w.NBT = (int)((T + PC_TB - 1) / PC_TB);
    const int PL = w.PL;
    w.o_redge = base;
    w.o_A = w.o_redge + pc_align((size_t)C * SC * sizeof(double));
    w.o_live = w.o_A + (with_A ? pc_align((size_t)SC * PL * PL * sizeof(double)) : 0);
    w.o_rowF = w.o_live + pc_align((size_t)SC * PL * sizeof(int32_t));
    w.o_F = w.o_rowF + pc_align((size_t)SC * PL * sizeof(double));
    w.o_mean = w.o_F + pc_align((size_t)SC * sizeof(double));
    w.o_isd = w.o_mean + pc_align((size_t)SC * Nreg * sizeof(double));
    w.o_q = w.o_isd + pc_align((size_t)SC * Nreg * sizeof(double));
    w.end = w.o_q + pc_align((size_t)SC * w.NBT * sizeof(double));
}

int fcd_corr_shrunk_at(fcd_ctx *ctx, const double *x, int64_t Sc, int64_t Nreg, int64_t T, const int32_t *n_frames, int64_t s0,
                       int64_t S_call, int shrink_mode, double shrink_value, const fcd_shrunk_ws &w, size_t edges_off, double *A,
                       double *alpha, int32_t *info, hipStream_t st) {
    const int64_t C = fcd_tri(Nreg);
    const int PL = w.PL, NBT = w.NBT;
    char *ws = (char *)ctx->ws.p;
    double *redge = (double *)(ws + w.o_redge), *Fsum = (double *)(ws + w.o_F);
    double *mean = (double *)(ws + w.o_mean), *isd = (double *)(ws + w.o_isd), *qpart = (double *)(ws + w.o_q);
    double *rowF = (double *)(ws + w.o_rowF);
    int32_t *live = (int32_t *)(ws + w.o_live);
    // the time slices of the correlation kernel follow the CALL's S, not the chunk's: the chunking changes no bit
    int rc = fcd_corr_edges_at(ctx, x, Sc, Nreg, T, 0, redge, edges_off, S_call, st);
    if (rc) return rc;
    const dim3 tgrid((unsigned)((C + 31) / 32), (unsigned)((Sc + 31) / 32));
    hipLaunchKernelGGL(pc_dense_kernel, tgrid, dim3(256), 0, st, redge, Sc, C, PL, A);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(pc_rows_kernel, dim3((unsigned)(PL / 4), (unsigned)Sc), dim3(256), 0, st, A, (int)Nreg, PL, live, rowF);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(pc_total_kernel, dim3((unsigned)Sc), dim3(64), 0, st, live, rowF, PL, (int)T, n_frames, s0, Fsum, info);
    FCD_LAUNCH_CHECK();
    if (shrink_mode == 1) {
        const int64_t rows = Sc * Nreg;
        hipLaunchKernelGGL(pc_moments_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, rows, (int)Nreg, PL, (int)T,
                           n_frames, s0, live, info, mean, isd);
        FCD_LAUNCH_CHECK();
        hipLaunchKernelGGL(pc_frame_kernel, dim3((unsigned)NBT, (unsigned)Sc), dim3(PC_TB), 0, st, x, (int)Nreg, (int)T, n_frames,
                           s0, mean, isd, NBT, qpart);
        FCD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pc_shrink_kernel, dim3((unsigned)PL, (unsigned)Sc), dim3(256), 0, st, A, (int)Nreg, PL, (int)T, n_frames, s0,
                       live, Fsum, qpart, NBT, shrink_mode, shrink_value, info, alpha);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_corr_partial(fcd_ctx *ctx, const double *ts, int64_t S, int64_t Nreg, int64_t T, const int32_t *n_frames,
                                int shrink_mode, double shrink_value, int fisher_z, double *out, double *alpha, int32_t *info,
                                fcd_stream stream) {
    if (!ctx || !ts || !out || !alpha || !info) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_corr_partial: null pointer");
    if (S < 1 || Nreg < 1 || T < 1) return fcd_fail(ctx, FCD_ERR_ARG, "fcd_corr_partial: need S, Nreg, T >= 1 (Nreg=%lld, T=%lld)", Nreg, T);
    if (shrink_mode != 0 && shrink_mode != 1) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_corr_partial: unknown shrink_mode %lld", shrink_mode);
    if (shrink_mode == 0 && !(shrink_value >= 0.0 && shrink_value <= 1.0))
        return fcd_fail(ctx, FCD_ERR_ARG, "fcd_corr_partial: shrink_value outside [0, 1]");
    if (Nreg > 1024) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_corr_partial: %lld regions, at most 1024", Nreg);
    if (Nreg < 2 || T < 2) return fcd_fail(ctx, FCD_ERR_SHAPE, "need S >= 1, Nreg >= 2, T >= 2 (Nreg=%lld, T=%lld)", Nreg, T);
    if (S > 65535 || T > INT32_MAX) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, "fcd_corr_partial: shape too large");
    if ((T & 1) == 0) FCD_ALIGN16(ctx, "fcd_corr_partial", "ts", ts);          // fcd_corr_edges' kernels read its rows as double2
    hipStream_t st = (hipStream_t)stream;
    const int64_t C = fcd_tri(Nreg);
    const int RT = (int)((Nreg + PNB - 1) / PNB), PL = RT * PNB;
    // subjects per chunk: the dense matrices stay below PC_MAT_BYTES (knob "partial_chunk": fewer, for tests)
    int64_t SC = (int64_t)(PC_MAT_BYTES / ((size_t)PL * PL * sizeof(double)));
    if (ctx->knobs.partial_chunk > 0 && SC > ctx->knobs.partial_chunk) SC = ctx->knobs.partial_chunk;
    if (SC < 1) SC = 1;
    if (SC > S) SC = S;
    // the kernel's LDS: the row panel [16][WLD] (WLD = 4 mod 16 doubles: rows 0, 4, 8, 12 + g of a fragment read fall on
    // different banks) and the inverse of the pivot block [16][17]
    const int WLD = PL + 4;
    const size_t shmem = ((size_t)PNB * WLD + PNB * 17) * sizeof(double);
    int rc = fcd_lds_attr(ctx, FCD_KA_PARTIAL, reinterpret_cast<const void *>(&pc_invert_kernel), shmem);
    if (rc) return rc;
    // this call's part of the workspace, in front of what the correlation kernels take (sized by the first, largest chunk):
    // the front half's (fcd_corr_shrunk_plan), then the inverse's diagonal
    fcd_shrunk_ws w;
    fcd_corr_shrunk_plan(SC, Nreg, T, 0, w);
    const size_t o_dinv = w.end;
    const size_t mine = o_dinv + pc_align((size_t)SC * PL * sizeof(double));
    rc = fcd_ws_reserve(ctx, mine + fcd_corr_edges_ws_bytes(ctx, SC, Nreg, T, S));
    if (rc) return rc;
    char *ws = (char *)ctx->ws.p;
    double *A = (double *)(ws + w.o_A), *dinv = (double *)(ws + o_dinv);
    const int32_t *live = (const int32_t *)(ws + w.o_live);
    const unsigned inv_threads = RT >= 8 ? 1024u : 256u;
    for (int64_t s0 = 0; s0 < S; s0 += SC) {
        const int64_t Sc = S - s0 < SC ? S - s0 : SC;
        rc = fcd_corr_shrunk_at(ctx, ts + s0 * Nreg * T, Sc, Nreg, T, n_frames, s0, S, shrink_mode, shrink_value, w, mine, A, alpha,
                                info, st);
        if (rc) return rc;
        const dim3 tgrid((unsigned)((C + 31) / 32), (unsigned)((Sc + 31) / 32));
        hipLaunchKernelGGL(pc_invert_kernel, dim3((unsigned)Sc), dim3(inv_threads), shmem, st, A, PL, RT, WLD, s0, info, dinv);
        FCD_LAUNCH_CHECK();
        hipLaunchKernelGGL(pc_emit_kernel, tgrid, dim3(256), 0, st, A, dinv, live, info, PL, Sc, s0, S, C, fisher_z ? 1 : 0, out);
        FCD_LAUNCH_CHECK();
    }
    return FCD_OK;
}
