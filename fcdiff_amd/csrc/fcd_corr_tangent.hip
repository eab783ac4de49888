// K_tangent: tangent-space connectivity fitted on the controls (fcd_tangent_fit, fcd_tangent_apply) and the batched symmetric
// eigensolver under it (fcd_sym_eigh).
//
// Not in the reference (its inputs are already correlations); oracle = tests/tangent_ref.py (numpy.longdouble Jacobi).
// include/fcdiff_hip.h has the rules in full.  Per subject the front half of fcd_corr_partial (fcd_corr_shrunk_at) gives the
// dense R_a = (1 - a) R + a I; then
//   M_s = W R_a,s W          two products on fp64 MFMA tiles, the second one's lower tiles mirrored   (tg_gemm_nt_kernel)
//   M_s = V L V^T            parallel cyclic Jacobi, one workgroup per matrix                         (eig_jacobi_kernel)
//   T_s = V log(L) V^T       the same product kernel with a diagonal in the middle                    (tg_fvals_kernel + gemm)
// and the fit wraps the fixed point of the Frechet mean round them.  Every product is  C = A diag(d) B^T  with both operands
// read along their rows: all the matrices that stand on the right here are symmetric (R_a, W, G^1/2) or V itself.
// Subjects are walked in chunks; no sum crosses a subject except the mean over the controls, which is a running sum in the
// order of the subjects, so the chunking changes no bit.  Every reduction has a fixed order; no floating-point atomics.
#include "fcd_common.h"

#include <math.h>

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int TNB = 16;                       // one MFMA tile
constexpr int EIG_LDS_N = 96;                 // up to here A and V^T live in LDS: 2 n (n | 1) doubles = 146 KB at 96
constexpr int EIG_MAX_SWEEPS = 40;            // the cap: a matrix that still rotates after so many sweeps gets status 2
constexpr double EIG_REL = 0x1p-58;           // an off-diagonal at or below this times ||A||_F is left alone
constexpr double TG_EIG_MIN = 1e-12;          // log, sqrt, 1/sqrt of an eigenvalue <= this times the largest: status 1
constexpr size_t TG_MAT_BYTES = (size_t)128 << 20;
enum { TG_F_LOG = 0, TG_F_EXP = 1, TG_F_SQRT = 2, TG_F_ISQRT = 3 };

__device__ __forceinline__ double tg_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// global stores of this wave have been acknowledged, then the barrier: the next phase of the SAME workgroup (same CU, same L1)
// reads what this one wrote
__device__ __forceinline__ void eig_sync() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// The eigensolver: two-sided parallel cyclic Jacobi, one workgroup per matrix, no word shared between workgroups.
// n <= EIG_LDS_N: A (n x n, leading dimension n | 1) and V^T in LDS; above, both in the workgroup's 2 n^2 doubles of `work`
// (the passes then go to the XCD's L2).  A sweep is m - 1 steps, m = n rounded up to even; step r pairs the indices by the
// circle method -- m - 1 sits still, the others turn -- so its m / 2 pairs are disjoint and their rotations commute; for odd
// n the index m - 1 does not exist and its partner has a bye.  A step is three phases with a barrier after each:
//   0  a thread per pair: the rotation (c, s) that zeroes A[p][q], skipped where |A[p][q]| <= EIG_REL ||A||_F, and the two new
//      diagonal entries a_pp - t a_pq, a_qq + t a_pq
//   1  columns p, q of every row of A
//   2  rows p, q of A and of V^T (row k of V^T is eigenvector k); the 2 x 2 block gets its exact values
// A sweep without a rotation ends the loop; EIG_MAX_SWEEPS bounds it.  Then the eigenvalues are ranked (ties by index), and
// w ascending and V (eigenvectors in columns) are written, with zeros in rows and columns n .. vpad - 1 of V for the callers
// that multiply whole tiles.  Only the lower triangle of the input is read; nothing at or beyond row or column n is.
// status: 0, 1 a non-finite entry (or a norm that overflows), 2 not converged; w and V are NaN where it is not 0.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void eig_jacobi_kernel(const double *__restrict__ Ain, int lda, int64_t sA, int n,
                                                          double *__restrict__ w, int ldw, double *__restrict__ Vout, int ldv,
                                                          int64_t sV, int vpad, int32_t *__restrict__ status, int sstride,
                                                          double *work, int in_lds) {
    extern __shared__ __attribute__((aligned(16))) double esm[];
    __shared__ double red[16];
    __shared__ int nrot;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, nt = (int)blockDim.x;
    const int ld = in_lds ? (n | 1) : n;
    const int m = (n + 1) & ~1, npair = m >> 1;
    double *A = in_lds ? esm : work + b * 2 * (int64_t)n * n;
    double *VT = A + (int64_t)n * ld;
    double *pc = in_lds ? esm + 2 * n * ld : esm;           // [npair] each: c, s, new a_pp, new a_qq; then p, q
    double *ps = pc + npair, *dp = ps + npair, *dq = dp + npair;
    int *pp = reinterpret_cast<int *>(dq + npair), *pq = pp + npair;
    const double *src = Ain + b * sA;
    double q2 = 0.0;
    for (int idx = tid; idx < n * n; idx += nt) {
        const int i = idx / n, j = idx - i * n;
        const double v = src[(int64_t)(i > j ? i : j) * lda + (i > j ? j : i)];
        A[i * ld + j] = v;
        VT[i * ld + j] = i == j ? 1.0 : 0.0;
        q2 += v * v;
    }
    q2 = fcd_wave_sum(q2);
    if ((tid & 63) == 0) red[tid >> 6] = q2;
    eig_sync();
    double nrm2 = 0.0;
    for (int k = 0; k < (nt >> 6); ++k) nrm2 += red[k];
    const bool finite = nrm2 < (double)INFINITY;             // (NaN: false)
    const double thr = EIG_REL * sqrt(nrm2);
    bool converged = false;
    if (finite) {
        for (int sweep = 0; sweep < EIG_MAX_SWEEPS; ++sweep) {
            if (tid == 0) nrot = 0;
            __syncthreads();
            for (int r = 0; r < m - 1; ++r) {
                for (int k = tid; k < npair; k += nt) {
                    const int a = k == 0 ? m - 1 : (r + k) % (m - 1);
                    const int c2 = k == 0 ? r : (r + (m - 1) - k) % (m - 1);
                    const int p = a < c2 ? a : c2, q = a < c2 ? c2 : a;
                    double c = 1.0, s = 0.0, ndp = 0.0, ndq = 0.0;
                    if (q < n) {
                        const double apq = A[p * ld + q];
                        if (fabs(apq) > thr) {
                            const double app = A[p * ld + p], aqq = A[q * ld + q];
                            const double theta = (aqq - app) / (2.0 * apq);
                            double t;
                            // (never taken: |apq| > 2^-58 ||A||_F and |aqq - app| <= 2 ||A||_F bound |theta| by 2^58)
                            if (fabs(theta) > 1e150) t = 0.5 / theta;
                            else t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                            c = 1.0 / sqrt(t * t + 1.0);
                            s = t * c;
                            ndp = app - t * apq;
                            ndq = aqq + t * apq;
                            if (s != 0.0) nrot = 1;
                        }
                    }
                    pc[k] = c, ps[k] = s, dp[k] = ndp, dq[k] = ndq;
                    pp[k] = p, pq[k] = q < n ? q : p;
                }
                eig_sync();
                for (int idx = tid; idx < npair * n; idx += nt) {
                    const int i = idx / npair, k = idx - i * npair;
                    const double s = ps[k];
                    if (s != 0.0) {
                        const double c = pc[k];
                        double *row = A + i * ld;
                        const int p = pp[k], q = pq[k];
                        const double x = row[p], y = row[q];
                        row[p] = c * x - s * y;
                        row[q] = s * x + c * y;
                    }
                }
                eig_sync();
                for (int idx = tid; idx < npair * n; idx += nt) {
                    const int k = idx / n, j = idx - k * n;
                    const double s = ps[k];
                    if (s != 0.0) {
                        const double c = pc[k];
                        const int p = pp[k], q = pq[k];
                        double *rp = A + p * ld, *rq = A + q * ld;
                        if (j == p) {
                            rp[j] = dp[k];
                            rq[j] = 0.0;
                        } else if (j == q) {
                            rp[j] = 0.0;
                            rq[j] = dq[k];
                        } else {
                            const double x = rp[j], y = rq[j];
                            rp[j] = c * x - s * y;
                            rq[j] = s * x + c * y;
                        }
                        double *vp = VT + p * ld, *vq = VT + q * ld;
                        const double vx = vp[j], vy = vq[j];
                        vp[j] = c * vx - s * vy;
                        vq[j] = s * vx + c * vy;
                    }
                }
                eig_sync();
            }
            const int any = nrot;
            __syncthreads();
            if (any == 0) {
                converged = true;
                break;
            }
        }
    }
    // the eigenvalues and their ranks: dd [n] and inv [n] over the pair arrays, which have had their day
    double *dd = pc;
    int *inv = reinterpret_cast<int *>(pc + m);
    const bool ok = finite && converged;
    for (int i = tid; i < n; i += nt) {
        dd[i] = A[i * ld + i];
        inv[i] = i;
    }
    eig_sync();
    int myrank = -1;
    if (ok && tid < n) {
        // (n <= 1024 = the largest workgroup; a smaller workgroup is launched only for n <= 32)
        const double di = dd[tid];
        int rk = 0;
        for (int j = 0; j < n; ++j) rk += (dd[j] < di || (dd[j] == di && j < tid)) ? 1 : 0;
        myrank = rk;
    }
    __syncthreads();
    if (myrank >= 0 && myrank < n) inv[myrank] = tid;
    __syncthreads();
    for (int r = tid; r < n; r += nt) w[b * ldw + r] = ok ? dd[inv[r]] : tg_nan();
    double *Vb = Vout + b * sV;
    for (int idx = tid; idx < vpad * vpad; idx += nt) {
        const int j = idx / vpad, r = idx - j * vpad;
        double v = 0.0;
        if (j < n && r < n) v = ok ? VT[inv[r] * ld + j] : tg_nan();
        Vb[(int64_t)j * ldv + r] = v;
    }
    if (tid == 0) status[b * sstride] = ok ? 0 : (finite ? 2 : 1);
}

// C_b = A_b diag(d_b) B_b^T on whole 16 x 16 tiles of PL x PL matrices (PL = 16 RT; d == nullptr: no diagonal).  A wave per
// tile of C, four to a workgroup; the k loop runs in order, four MFMAs per 16 columns, MFMA g taking columns 4 (l >> 4) + g of
// both operands (fcd_corr_partial.hip has the fragment layout), so a lane's four values of either operand are 32 contiguous
// bytes of a row.  sym: only the tiles I >= J are computed and each element is stored at (i, j) and (j, i) -- the diagonal tile
// keeps its own lower half -- so C is symmetric bit for bit.  A stride of 0 shares an operand over the batch.
__global__ __launch_bounds__(256) void tg_gemm_nt_kernel(const double *__restrict__ A, int64_t sA, const double *__restrict__ B,
                                                         int64_t sB, const double *__restrict__ d, int64_t sd,
                                                         double *__restrict__ C, int64_t sC, int PL, int RT, int sym) {
    const int64_t b = blockIdx.y;
    const int l = threadIdx.x & 63;
    const int t = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (t >= RT * RT) return;
    const int I = t / RT, J = t - I * RT;
    if (sym && J > I) return;
    const int i16 = l & 15, kq = l >> 4;
    const double *ap = A + b * sA + (int64_t)(I * TNB + i16) * PL + kq * 4;
    const double *bp = B + b * sB + (int64_t)(J * TNB + i16) * PL + kq * 4;
    const double *dv = d ? d + b * sd + kq * 4 : nullptr;
    double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < PL; k0 += TNB) {
        const double2 a01 = *reinterpret_cast<const double2 *>(ap + k0), a23 = *reinterpret_cast<const double2 *>(ap + k0 + 2);
        const double2 b01 = *reinterpret_cast<const double2 *>(bp + k0), b23 = *reinterpret_cast<const double2 *>(bp + k0 + 2);
        double fa[4] = {a01.x, a01.y, a23.x, a23.y};
        const double fb[4] = {b01.x, b01.y, b23.x, b23.y};
        if (dv) {
#pragma unroll
            for (int g = 0; g < 4; ++g) fa[g] *= dv[k0 + g];
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[g], fb[g], acc, 0, 0, 0);
    }
    double *Cb = C + b * sC;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = I * TNB + kq + 4 * r, j = J * TNB + i16;
        if (!sym) {
            Cb[(int64_t)i * PL + j] = acc[r];
        } else if (i >= j) {
            Cb[(int64_t)i * PL + j] = acc[r];
            Cb[(int64_t)j * PL + i] = acc[r];
        }
    }
}

// f(w) of one matrix per workgroup -> fv (B, PL), zero behind n, and the matrix's status: 5 where the eigensolver gave up
// (estat != 0), 1 where log, sqrt or 1 / sqrt meets an eigenvalue <= TG_EIG_MIN times the largest.  The status word is only
// set where it was 0; fv is NaN where it is set here.
__global__ __launch_bounds__(256) void tg_fvals_kernel(const double *__restrict__ w, int n, int PL, int func,
                                                       const int32_t *__restrict__ estat, double *__restrict__ fv,
                                                       int32_t *__restrict__ status, int sstride) {
    const int64_t b = blockIdx.x;
    const double *wb = w + b * PL;
    int bad = estat[b] != 0 ? 5 : 0;
    if (!bad && func != TG_F_EXP && !(wb[0] > TG_EIG_MIN * wb[n - 1])) bad = 1;
    for (int k = threadIdx.x; k < PL; k += 256) {
        double v = 0.0;
        if (k < n) {
            const double x = wb[k];
            if (bad) v = tg_nan();
            else if (func == TG_F_LOG) v = log(x);
            else if (func == TG_F_EXP) v = exp(x);
            else if (func == TG_F_SQRT) v = sqrt(x);
            else v = 1.0 / sqrt(x);
        }
        fv[b * PL + k] = v;
    }
    if (threadIdx.x == 0 && bad && status[b * sstride] == 0) status[b * sstride] = bad;
}

// a subject with a dead region: status 4 (a matrix function acts on the whole matrix)
__global__ __launch_bounds__(256) void tg_dead_kernel(int32_t *__restrict__ info, int64_t s_base, int64_t Sc, int Nreg) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= Sc) return;
    int32_t *p = info + (s_base + s) * 2;
    if (p[1] == 0 && p[0] < Nreg) p[1] = 4;
}

__global__ __launch_bounds__(256) void tg_used_kernel(const int32_t *__restrict__ info, int64_t H, uint8_t *__restrict__ used) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < H) used[s] = info[s * 2 + 1] == 0 ? 1 : 0;
}

// acc[e] = (first ? 0 : acc[e]) + sum over the used subjects of the chunk, in their order, of X[s][e]: a running sum, so the
// chunk boundaries change no bit; scale != 0 then divides by it
__global__ __launch_bounds__(256) void tg_accum_kernel(const double *__restrict__ X, int64_t Sc, int64_t n2,
                                                       const uint8_t *__restrict__ used, int first, double scale,
                                                       double *__restrict__ acc) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n2) return;
    double a = first ? 0.0 : acc[e];
    for (int64_t s = 0; s < Sc; ++s) {
        if (used[s]) a += X[s * n2 + e];
    }
    acc[e] = scale != 0.0 ? a / scale : a;
}

// Frobenius norm of the n x n block of a PL-padded matrix: one workgroup, a thread's elements in order, the wave's tree, the
// waves in order
__global__ __launch_bounds__(1024) void tg_norm_kernel(const double *__restrict__ X, int n, int PL, double *__restrict__ out) {
    __shared__ double red[16];
    const int tid = threadIdx.x;
    double q = 0.0;
    for (int idx = tid; idx < n * n; idx += 1024) {
        const int i = idx / n, j = idx - i * n;
        const double v = X[(int64_t)i * PL + j];
        q += v * v;
    }
    q = fcd_wave_sum(q);
    if ((tid & 63) == 0) red[tid >> 6] = q;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += red[k];
        out[0] = sqrt(t);
    }
}

// (n, n) <-> the n x n block of a (PL, PL) matrix whose padding is zero
__global__ __launch_bounds__(256) void tg_pad_kernel(const double *__restrict__ src, int n, int PL, double *__restrict__ dst) {
    const int idx = (int)blockIdx.x * 256 + threadIdx.x;
    if (idx >= PL * PL) return;
    const int i = idx / PL, j = idx - i * PL;
    dst[idx] = (i < n && j < n) ? src[(int64_t)i * n + j] : 0.0;
}
__global__ __launch_bounds__(256) void tg_unpad_kernel(const double *__restrict__ src, int n, int PL, double *__restrict__ dst) {
    const int idx = (int)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * n) return;
    const int i = idx / n, j = idx - i * n;
    dst[idx] = src[(int64_t)i * PL + j];
}

// T_s back into edge-major (C, S): the reads run along m within a row, the stores along s (pc_emit_kernel's tile)
__global__ __launch_bounds__(256) void tg_emit_kernel(const double *__restrict__ Tm, const int32_t *__restrict__ info, int PL,
                                                      int64_t Sc, int64_t s_base, int64_t S, int64_t C, double *__restrict__ out) {
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
        double v = tg_nan();
        if (info[(s_base + s) * 2 + 1] == 0) v = Tm[(s * PL + n) * PL + m];
        tile[ty + j][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int64_t cc = c0 + ty + j, s = s0 + tx;
        if (s < Sc && cc < C) out[cc * S + s_base + s] = tile[tx][ty + j];
    }
}
// ... and its diagonal into (Nreg, S)
__global__ __launch_bounds__(256) void tg_diag_kernel(const double *__restrict__ Tm, const int32_t *__restrict__ info, int PL,
                                                      int Nreg, int64_t Sc, int64_t s_base, int64_t S, double *__restrict__ diag) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)Nreg * Sc) return;
    const int64_t i = idx / Sc, s = idx - i * Sc;
    double v = tg_nan();
    if (info[(s_base + s) * 2 + 1] == 0) v = Tm[(s * PL + i) * PL + i];
    diag[i * S + s_base + s] = v;
}

inline size_t tg_align(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- host: launches -------------------------------------------------------------------------------------------------------
size_t eig_work_bytes(int64_t B, int n) { return n > EIG_LDS_N ? (size_t)B * 2 * n * n * sizeof(double) : 0; }

int eig_launch(fcd_ctx *ctx, hipStream_t st, const double *A, int lda, int64_t sA, int n, int64_t B, double *w, int ldw, double *V,
               int ldv, int64_t sV, int vpad, int32_t *status, int sstride, double *work) {
    const int in_lds = n <= EIG_LDS_N ? 1 : 0;
    const int npair = ((n + 1) & ~1) >> 1;
    const size_t shmem = (in_lds ? (size_t)2 * n * (n | 1) * sizeof(double) : 0) + (size_t)npair * (4 * sizeof(double) + 2 * sizeof(int));
    int rc = fcd_lds_attr(ctx, FCD_KA_EIGH, reinterpret_cast<const void *>(&eig_jacobi_kernel), shmem);
    if (rc) return rc;
    hipLaunchKernelGGL(eig_jacobi_kernel, dim3((unsigned)B), dim3(n <= 32 ? 256u : 1024u), shmem, st, A, lda, sA, n, w, ldw, V, ldv,
                       sV, vpad, status, sstride, work, in_lds);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

int gemm_launch(hipStream_t st, const double *A, int64_t sA, const double *B, int64_t sB, const double *d, int64_t sd, double *C,
                int64_t sC, int PL, int64_t batch, int sym) {
    const int RT = PL / TNB;
    hipLaunchKernelGGL(tg_gemm_nt_kernel, dim3((unsigned)((RT * RT + 3) / 4), (unsigned)batch), dim3(256), 0, st, A, sA, B, sB, d, sd,
                       C, sC, PL, RT, sym);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

// the scratch of a chunk of CH matrices (and of the single matrices of the fit, which use slot 0 between the chunks)
struct tg_bufs {
    double *Y, *M, *V, *work, *wv, *fv;
    int32_t *estat;
    int PL, n;
};
size_t tg_bufs_plan(int64_t CH, int n, int PL, size_t base, size_t off[7]) {
    const size_t mat = tg_align((size_t)CH * PL * PL * sizeof(double)), vec = tg_align((size_t)CH * PL * sizeof(double));
    off[0] = base;
    off[1] = off[0] + mat;
    off[2] = off[1] + mat;
    off[3] = off[2] + mat;
    off[4] = off[3] + tg_align(eig_work_bytes(CH, n));
    off[5] = off[4] + vec;
    off[6] = off[5] + vec;
    return off[6] + tg_align((size_t)CH * sizeof(int32_t));
}
tg_bufs tg_bufs_at(char *ws, const size_t off[7], int n, int PL) {
    tg_bufs b;
    b.Y = (double *)(ws + off[0]), b.M = (double *)(ws + off[1]), b.V = (double *)(ws + off[2]), b.work = (double *)(ws + off[3]);
    b.wv = (double *)(ws + off[4]), b.fv = (double *)(ws + off[5]), b.estat = (int32_t *)(ws + off[6]);
    b.PL = PL, b.n = n;
    return b;
}

// F_b = f(X_b) for `batch` symmetric PL-padded matrices X -> F (may be b.Y or b.M, not X itself and not b.V); status words at
// status[b * sstride].  F2 != nullptr: a second function f2 of the same matrices from the same decomposition -> F2.
int tg_matfunc(fcd_ctx *ctx, hipStream_t st, const tg_bufs &b, const double *X, int64_t batch, int func, double *F, int32_t *status,
               int sstride, int func2 = 0, double *F2 = nullptr) {
    const int PL = b.PL, n = b.n;
    const int64_t P2 = (int64_t)PL * PL;
    int rc = eig_launch(ctx, st, X, PL, P2, n, batch, b.wv, PL, b.V, PL, P2, PL, b.estat, 1, b.work);
    if (rc) return rc;
    hipLaunchKernelGGL(tg_fvals_kernel, dim3((unsigned)batch), dim3(256), 0, st, b.wv, n, PL, func, b.estat, b.fv, status, sstride);
    FCD_LAUNCH_CHECK();
    rc = gemm_launch(st, b.V, P2, b.V, P2, b.fv, PL, F, P2, PL, batch, 1);
    if (rc || !F2) return rc;
    hipLaunchKernelGGL(tg_fvals_kernel, dim3((unsigned)batch), dim3(256), 0, st, b.wv, n, PL, func2, b.estat, b.fv, status, sstride);
    FCD_LAUNCH_CHECK();
    return gemm_launch(st, b.V, P2, b.V, P2, b.fv, PL, F2, P2, PL, batch, 1);
}

// T_s = logm(W A_s W) for a chunk -> b.Y; the subjects' status words are info[(s0 + s) * 2 + 1]
int tg_log_chunk(fcd_ctx *ctx, hipStream_t st, const tg_bufs &b, const double *A, const double *Wp, int64_t Sc, int32_t *info,
                 int64_t s0) {
    const int PL = b.PL;
    const int64_t P2 = (int64_t)PL * PL;
    int rc = gemm_launch(st, Wp, 0, A, P2, nullptr, 0, b.Y, P2, PL, Sc, 0);          // Y = W A      (A symmetric)
    if (rc) return rc;
    rc = gemm_launch(st, b.Y, P2, Wp, 0, nullptr, 0, b.M, P2, PL, Sc, 1);            // M = Y W      (W symmetric), mirrored
    if (rc) return rc;
    return tg_matfunc(ctx, st, b, b.M, Sc, TG_F_LOG, b.Y, info + s0 * 2 + 1, 2);
}

int tg_check(fcd_ctx *ctx, const fcd_tangent_desc *d, const char *who) {
    if (!ctx) return FCD_ERR_ARG;
    if (!d) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null descriptor");
    if (d->size != sizeof(fcd_tangent_desc))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "descriptor size %lld, this library's is %lld", d->size, (long long)sizeof(fcd_tangent_desc));
    if (d->flags & ~(uint32_t)FCD_TANGENT_EUCLIDEAN) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "unknown flags %lld", d->flags);
    if (!d->ts || !d->alpha || !d->info || !d->W) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    if (d->S < 1 || d->Nreg < 1 || d->T < 1)
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "need S, Nreg, T >= 1 (Nreg=%lld, T=%lld)", d->Nreg, d->T);
    if (d->shrink_mode != 0 && d->shrink_mode != 1) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "unknown shrink_mode %lld", d->shrink_mode);
    if (d->shrink_mode == 0 && !(d->shrink_value >= 0.0 && d->shrink_value <= 1.0))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "shrink_value outside [0, 1]");
    if (d->Nreg > 1024) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "%lld regions, at most 1024", d->Nreg);
    if (d->Nreg < 2 || d->T < 2) return fcd_fail_who(ctx, FCD_ERR_SHAPE, who, "need Nreg >= 2, T >= 2 (Nreg=%lld, T=%lld)", d->Nreg, d->T);
    if (d->S > 65535 || d->T > INT32_MAX) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "shape too large (S=%lld, T=%lld)", d->S, d->T);
    if ((d->T & 1) == 0) FCD_ALIGN16(ctx, who, "ts", d->ts);          // fcd_corr_edges' kernels read its rows as double2
    return FCD_OK;
}

int64_t tg_chunk(const fcd_ctx *ctx, int PL, int64_t S) {
    int64_t SC = (int64_t)(TG_MAT_BYTES / ((size_t)PL * PL * sizeof(double)));
    if (ctx->knobs.tangent_chunk > 0 && SC > ctx->knobs.tangent_chunk) SC = ctx->knobs.tangent_chunk;
    if (SC < 1) SC = 1;
    return SC > S ? S : SC;
}

}  // namespace

extern "C" int fcd_sym_eigh(fcd_ctx *ctx, const fcd_eigh_desc *d) {
    static const char *who = "fcd_sym_eigh";
    if (!ctx) return FCD_ERR_ARG;
    if (!d) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null descriptor");
    if (d->size != sizeof(fcd_eigh_desc))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "descriptor size %lld, this library's is %lld", d->size, (long long)sizeof(fcd_eigh_desc));
    if (d->flags) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "unknown flags %lld", d->flags);
    if (!d->A || !d->w || !d->V || !d->status) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    if (d->B < 1 || d->n < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "need B, n >= 1 (B=%lld, n=%lld)", d->B, d->n);
    if (d->n > 1024) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "n=%lld, at most 1024", d->n);
    if (d->B > ((int64_t)1 << 24)) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "B=%lld matrices, at most 2^24", d->B);
    hipStream_t st = (hipStream_t)d->stream;
    const int n = (int)d->n;
    const int64_t n2 = (int64_t)n * n;
    int64_t BC = (int64_t)(4 * TG_MAT_BYTES / ((size_t)2 * n2 * sizeof(double)));
    if (ctx->knobs.tangent_chunk > 0 && BC > ctx->knobs.tangent_chunk) BC = ctx->knobs.tangent_chunk;
    if (BC < 1) BC = 1;
    if (BC > d->B) BC = d->B;
    int rc = fcd_ws_reserve(ctx, eig_work_bytes(BC, n));
    if (rc) return rc;
    for (int64_t b0 = 0; b0 < d->B; b0 += BC) {
        const int64_t Bc = d->B - b0 < BC ? d->B - b0 : BC;
        rc = eig_launch(ctx, st, d->A + b0 * n2, n, n2, n, Bc, d->w + b0 * n, n, d->V + b0 * n2, n, n2, n, d->status + b0, 1,
                        (double *)ctx->ws.p);
        if (rc) return rc;
    }
    return FCD_OK;
}

extern "C" int fcd_tangent_apply(fcd_ctx *ctx, const fcd_tangent_desc *d) {
    static const char *who = "fcd_tangent_apply";
    int rc = tg_check(ctx, d, who);
    if (rc) return rc;
    if (!d->out || !d->diag) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    hipStream_t st = (hipStream_t)d->stream;
    const int64_t S = d->S, Nreg = d->Nreg, T = d->T, C = fcd_tri(Nreg);
    const int n = (int)Nreg, PL = (int)((Nreg + TNB - 1) / TNB) * TNB;
    const int64_t P2 = (int64_t)PL * PL;
    const int64_t SC = tg_chunk(ctx, PL, S);
    fcd_shrunk_ws w;
    fcd_corr_shrunk_plan(SC, Nreg, T, 0, w);
    const size_t o_W = w.end;
    size_t off[7];
    const size_t mine = tg_bufs_plan(SC, n, PL, o_W + tg_align((size_t)P2 * sizeof(double)), off);
    rc = fcd_ws_reserve(ctx, mine + fcd_corr_edges_ws_bytes(ctx, SC, Nreg, T, S));
    if (rc) return rc;
    char *ws = (char *)ctx->ws.p;
    double *A = (double *)(ws + w.o_A), *Wp = (double *)(ws + o_W);
    const tg_bufs b = tg_bufs_at(ws, off, n, PL);
    hipLaunchKernelGGL(tg_pad_kernel, dim3((unsigned)((P2 + 255) / 256)), dim3(256), 0, st, d->W, n, PL, Wp);
    FCD_LAUNCH_CHECK();
    for (int64_t s0 = 0; s0 < S; s0 += SC) {
        const int64_t Sc = S - s0 < SC ? S - s0 : SC;
        rc = fcd_corr_shrunk_at(ctx, d->ts + s0 * Nreg * T, Sc, Nreg, T, d->n_frames, s0, S, d->shrink_mode, d->shrink_value, w, mine, A,
                                d->alpha, d->info, st);
        if (rc) return rc;
        hipLaunchKernelGGL(tg_dead_kernel, dim3((unsigned)((Sc + 255) / 256)), dim3(256), 0, st, d->info, s0, Sc, n);
        FCD_LAUNCH_CHECK();
        rc = tg_log_chunk(ctx, st, b, A, Wp, Sc, d->info, s0);
        if (rc) return rc;
        const dim3 tgrid((unsigned)((C + 31) / 32), (unsigned)((Sc + 31) / 32));
        hipLaunchKernelGGL(tg_emit_kernel, tgrid, dim3(256), 0, st, b.Y, d->info, PL, Sc, s0, S, C, d->out);
        FCD_LAUNCH_CHECK();
        hipLaunchKernelGGL(tg_diag_kernel, dim3((unsigned)((Nreg * Sc + 255) / 256)), dim3(256), 0, st, b.Y, d->info, PL, n, Sc, s0, S,
                           d->diag);
        FCD_LAUNCH_CHECK();
    }
    return FCD_OK;
}

extern "C" int fcd_tangent_fit(fcd_ctx *ctx, const fcd_tangent_desc *d) {
    static const char *who = "fcd_tangent_fit";
    int rc = tg_check(ctx, d, who);
    if (rc) return rc;
    if (!d->G || !d->G_half || !d->used || !d->n_iter || !d->grad_norm) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    const bool geometric = !(d->flags & FCD_TANGENT_EUCLIDEAN);
    if (geometric && !(d->tol > 0.0)) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "tol must be > 0");
    if (geometric && d->max_iter < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "max_iter=%lld must be >= 1", d->max_iter);
    hipStream_t st = (hipStream_t)d->stream;
    const int64_t H = d->S, Nreg = d->Nreg, T = d->T;
    const int n = (int)Nreg, PL = (int)((Nreg + TNB - 1) / TNB) * TNB;
    const int64_t P2 = (int64_t)PL * PL;
    const int64_t SC = tg_chunk(ctx, PL, H);
    // workspace: the front half's | R_a of every control | G, G^1/2, W, Tbar (padded) | norm, status word | the chunk's scratch
    fcd_shrunk_ws w;
    fcd_corr_shrunk_plan(SC, Nreg, T, 0, w, false);               // (R_a goes straight into RA: no slot of the plan's for it)
    const size_t mat = tg_align((size_t)P2 * sizeof(double));
    const size_t o_RA = w.end, o_G = o_RA + tg_align((size_t)H * P2 * sizeof(double));
    const size_t o_Gh = o_G + mat, o_W = o_Gh + mat, o_Tb = o_W + mat, o_sc = o_Tb + mat;
    size_t off[7];
    const size_t mine = tg_bufs_plan(SC, n, PL, o_sc + 256, off);
    if (mine > ((size_t)64 << 30)) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "H=%lld controls of %lld regions need more than 64 GiB", H, Nreg);
    rc = fcd_ws_reserve(ctx, mine + fcd_corr_edges_ws_bytes(ctx, SC, Nreg, T, H));
    if (rc) return rc;
    char *ws = (char *)ctx->ws.p;
    double *RA = (double *)(ws + o_RA), *Gp = (double *)(ws + o_G), *Ghp = (double *)(ws + o_Gh), *Wp = (double *)(ws + o_W);
    double *Tb = (double *)(ws + o_Tb), *norm_d = (double *)(ws + o_sc);
    int32_t *gstat = (int32_t *)(ws + o_sc + 8);
    const tg_bufs b = tg_bufs_at(ws, off, n, PL);
    const unsigned g2 = (unsigned)((P2 + 255) / 256);
    FCD_HIP_TRY(hipMemsetAsync(gstat, 0, sizeof(int32_t), st));
    // 1  R_a of every control, its status (4: a dead region; 1: lambda_min(R_a) <= 1e-12 lambda_max), and who is used
    for (int64_t s0 = 0; s0 < H; s0 += SC) {
        const int64_t Sc = H - s0 < SC ? H - s0 : SC;
        rc = fcd_corr_shrunk_at(ctx, d->ts + s0 * Nreg * T, Sc, Nreg, T, d->n_frames, s0, H, d->shrink_mode, d->shrink_value, w, mine,
                                RA + s0 * P2, d->alpha, d->info, st);
        if (rc) return rc;
        hipLaunchKernelGGL(tg_dead_kernel, dim3((unsigned)((Sc + 255) / 256)), dim3(256), 0, st, d->info, s0, Sc, n);
        FCD_LAUNCH_CHECK();
        rc = eig_launch(ctx, st, RA + s0 * P2, PL, P2, n, Sc, b.wv, PL, b.V, PL, P2, PL, b.estat, 1, b.work);
        if (rc) return rc;
        hipLaunchKernelGGL(tg_fvals_kernel, dim3((unsigned)Sc), dim3(256), 0, st, b.wv, n, PL, (int)TG_F_LOG, b.estat, b.fv,
                           d->info + s0 * 2 + 1, 2);
        FCD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tg_used_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, st, d->info, H, d->used);
    FCD_LAUNCH_CHECK();
    int64_t n_used = 0;
    {
        uint8_t *hu = new uint8_t[(size_t)H];
        hipError_t e = hipMemcpyAsync(hu, d->used, (size_t)H, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        for (int64_t s = 0; s < H; ++s) n_used += hu[s];
        delete[] hu;
        if (e != hipSuccess) return (int)e;
    }
    *d->n_iter = 0;
    *d->grad_norm = NAN;
    if (n_used < 2) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "%lld usable controls of %lld, at least 2 are needed", n_used, H);
    // 2  the Euclidean mean, in the order of the controls
    for (int64_t s0 = 0; s0 < H; s0 += SC) {
        const int64_t Sc = H - s0 < SC ? H - s0 : SC;
        hipLaunchKernelGGL(tg_accum_kernel, dim3(g2), dim3(256), 0, st, RA + s0 * P2, Sc, P2, d->used + s0, s0 == 0 ? 1 : 0,
                           s0 + Sc == H ? (double)n_used : 0.0, Gp);
        FCD_LAUNCH_CHECK();
    }
    // 3  G^1/2 and W = G^-1/2; geometric: the fixed point
    int it = 0;
    bool converged = !geometric;
    double nrm = NAN;
    int32_t gs = 0;
    for (;;) {
        rc = tg_matfunc(ctx, st, b, Gp, 1, TG_F_SQRT, Ghp, gstat, 1, TG_F_ISQRT, Wp);        // one decomposition of G for both
        if (rc) return rc;
        if (!geometric) break;
        ++it;
        for (int64_t s0 = 0; s0 < H; s0 += SC) {
            const int64_t Sc = H - s0 < SC ? H - s0 : SC;
            // (status words of the controls: a control that was usable and fails here turns the norm NaN and is reported)
            rc = tg_log_chunk(ctx, st, b, RA + s0 * P2, Wp, Sc, d->info, s0);
            if (rc) return rc;
            hipLaunchKernelGGL(tg_accum_kernel, dim3(g2), dim3(256), 0, st, b.Y, Sc, P2, d->used + s0, s0 == 0 ? 1 : 0,
                               s0 + Sc == H ? (double)n_used : 0.0, Tb);
            FCD_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(tg_norm_kernel, dim3(1), dim3(1024), 0, st, Tb, n, PL, norm_d);
        FCD_LAUNCH_CHECK();
        double host[2];                                     // the norm and, behind it, the status word of the single matrices
        FCD_HIP_TRY(hipMemcpyAsync(host, norm_d, sizeof(host), hipMemcpyDeviceToHost, st));
        FCD_HIP_TRY(hipStreamSynchronize(st));
        nrm = host[0];
        memcpy(&gs, &host[1], sizeof(gs));
        if (gs != 0) break;
        if (nrm <= d->tol * sqrt((double)Nreg)) {
            converged = true;
            break;
        }
        if (it >= d->max_iter || !(nrm == nrm)) break;
        // G <- G^1/2 expm(Tbar) G^1/2
        rc = tg_matfunc(ctx, st, b, Tb, 1, TG_F_EXP, b.M, gstat, 1);
        if (rc) return rc;
        rc = gemm_launch(st, Ghp, 0, b.M, 0, nullptr, 0, b.Y, 0, PL, 1, 0);            // Y = G^1/2 E   (E symmetric)
        if (rc) return rc;
        rc = gemm_launch(st, b.Y, 0, Ghp, 0, nullptr, 0, Gp, 0, PL, 1, 1);             // G = Y G^1/2, mirrored
        if (rc) return rc;
    }
    if (!geometric) {
        FCD_HIP_TRY(hipMemcpyAsync(&gs, gstat, sizeof(gs), hipMemcpyDeviceToHost, st));
        FCD_HIP_TRY(hipStreamSynchronize(st));
    }
    const unsigned gn = (unsigned)(((int64_t)n * n + 255) / 256);
    hipLaunchKernelGGL(tg_unpad_kernel, dim3(gn), dim3(256), 0, st, Gp, n, PL, d->G);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(tg_unpad_kernel, dim3(gn), dim3(256), 0, st, Ghp, n, PL, d->G_half);
    FCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(tg_unpad_kernel, dim3(gn), dim3(256), 0, st, Wp, n, PL, d->W);
    FCD_LAUNCH_CHECK();
    *d->n_iter = converged ? it : -it;
    *d->grad_norm = nrm;
    if (gs != 0)
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "the reference is not positive definite to 1e-12 or its decomposition failed (status %lld, iteration %lld)", gs, it);
    return FCD_OK;
}
