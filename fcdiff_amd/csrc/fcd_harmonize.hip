// K_harm: site harmonisation (ComBat) fitted on the controls (fcd_site_harmonize_fit, fcd_site_harmonize_apply).
//
// Per connection c over the controls observed there (all of them without FCD_DATA_NAN_MISSING), i(h) the site of control h:
//   1. ybar_i = mean of site i;  e_h = (y_h - ybar_i(h)) - sum_q d_q W[h,q],  d = W^T y  (W orthonormal, its columns centred
//      within every site, so W^T y is W^T of the site-centred row);  beta = T d;  sigma2 = sum_h e_h^2 / n, from the residuals;
//   2. alpha_i = ybar_i - (zbar_i - z_ref) . beta;  abar = sum_i (n_i / n) alpha_i;  gamma_hat_i = (alpha_i - abar) / sigma;
//      delta2_hat_i = sum_{h in i} e_h^2 / (sigma2 (n_i - 1));
//   3. fitted iff n - B_c - Q' >= 1 and sum e^2 > 0 (status 0); otherwise every real output of the connection is NaN, its
//      shift 0 and its scale 1, which fcd_site_harmonize_apply copies through;
//   4. per site over the fitted connections: mean and variance (ddof 1) of gamma_hat and of delta2_hat, each in two passes;
//   5. the fixed point of ComBat's empirical-Bayes map per (site, fitted connection), from sufficient statistics alone;
//   6. shift = sigma gamma_star, scale = sqrt(delta2_star).
//
// Kernels (caller's stream, fixed summation orders, no floating-point atomics: two calls agree bit for bit):
//   harm_upload_kernel  the small host arrays of the design (T, zbar - z_ref) travel as kernel arguments, 128 doubles a launch,
//                       into the context's workspace: no copy that could wait for the stream, no pinned buffer to reuse.
//   harm_fit_kernel     one wave per connection, four to a workgroup, a workgroup walks many connections.  Site ids and W are
//                       staged in LDS once per workgroup (W where H Q' <= 2048, else it is read through the cache).  A row is
//                       read from memory once into the wave's LDS row (256 controls at a time; a longer row is read again from
//                       cache for the residuals).  LANES OWN SITES: with Bp = B rounded up to a power of two, lane l is group
//                       l / Bp of site l % Bp; it walks every (64 / Bp)-th staged control in order and adds those of its
//                       site, and a butterfly over the group bits joins a site's groups: the order of a site's sum depends
//                       on B and the row alone, never on the launch shape.  Column q of W^T y the same way, 8 lanes a column.
//                       Then the residuals with lanes over the controls, and the sites' sums of their squares as before.
//                       No workgroup barrier after the staging.
//   harm_prior_kernel   one workgroup per site over the (B, C) planes: count, mean, centred squares, by LDS trees.
//   harm_eb_kernel      one lane per (site, connection): the scalar iteration.
//   harm_apply_kernel   out = ((x - m) - shift) / scale + m, m = abar + sum_q beta[c,q] (z[s,q] - z_ref[q]): a workgroup stages
//                       z - z_ref and the site ids of 256 subjects and the shift / scale of 32 connections, 16 bytes per lane
//                       where the shape allows.  A pair with shift 0 and scale 1 is copied (the same bits).
#include "fcd_common.h"

#include <float.h>

namespace {

constexpr int HB = 64;                   // sites: one lane each
constexpr int HQ = 8;                    // covariate columns
constexpr int HH = 4096;                 // controls: the site ids of all of them are staged
constexpr int HC = 256;                  // controls of a row staged per wave at once
constexpr int HW = 2048;                 // doubles of W staged per workgroup
constexpr int FIT_WAVES = 4;
constexpr int EB_MAX_STEPS = 1000;
constexpr double EB_TOL = 1e-13;

enum { ST_FITTED = 0, ST_DOF = 1, ST_CONSTANT = 2, ST_NAN = 3, ST_SITE = 4 };

__device__ __forceinline__ void harm_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct harm_chunk {
    double v[128];
};
__global__ __launch_bounds__(128) void harm_upload_kernel(harm_chunk ch, double *__restrict__ dst, int n) {
    const int t = threadIdx.x;
    if (t < n) dst[t] = ch.v[t];
}

struct harm_fit_args {
    const double *b;
    const unsigned char *site;
    const double *W;             // (H, Qp)
    const double *T;             // (Q, Qp), workspace
    const double *M;             // (B, Q) zbar - z_ref, workspace
    int64_t C;
    int H, B, Q, Qp, missing;
    double *grand_mean, *pooled_sd, *beta, *gamma_hat, *delta2_hat;
    int32_t *n_obs, *info;
    volatile unsigned *err;
};

__global__ __launch_bounds__(64 * FIT_WAVES) void harm_fit_kernel(const harm_fit_args a) {
    __shared__ unsigned char s_site[HH];
    __shared__ double s_W[HW];
    __shared__ double s_row[FIT_WAVES][HC];
    __shared__ double s_ybar[FIT_WAVES][HB];
    __shared__ double s_d[FIT_WAVES][HQ];
    __shared__ double s_beta[FIT_WAVES][HQ];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = a.H, B = a.B, Q = a.Q, Qp = a.Qp;
    const bool missing = a.missing != 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int h = tid; h < H; h += 64 * FIT_WAVES) {
        const unsigned char s = a.site[h];
        s_site[h] = s;
        if ((int)s >= B) s_bad = 1;
    }
    const bool w_staged = H * Qp <= HW;
    if (w_staged)
        for (int e = tid; e < H * Qp; e += 64 * FIT_WAVES) s_W[e] = a.W[e];
    __syncthreads();
    const bool bad = s_bad != 0;
    if (bad && blockIdx.x == 0 && tid == 0)
        __hip_atomic_store(const_cast<unsigned *>(a.err), FCD_DEV_ERR_HARM_SITE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const double *Wp = w_staged ? s_W : a.W;
    double *row = s_row[wv];
    // lane = (group, site): Bp = B rounded up to a power of two, SG = 64 / Bp groups; group g of site i takes the controls
    // g, g + SG, ... of every staged piece, and a butterfly over the group bits joins them.  The same for W's columns, 8 to a group.
    int Bp = 1;
    while (Bp < B) Bp <<= 1;
    const int SG = 64 / Bp, my_site = lane & (Bp - 1), sg = lane / Bp, my_q = lane & (HQ - 1), qg = lane / HQ;
    const double nan = __builtin_nan("");
    const int64_t stride = (int64_t)gridDim.x * FIT_WAVES;
    for (int64_t c = (int64_t)blockIdx.x * FIT_WAVES + wv; c < a.C; c += stride) {
        const double *__restrict__ y = a.b + c * H;
        double sum = 0.0, dacc = 0.0, sse_i = 0.0;
        int n_i = 0;
        if (!bad) {
            // the site's sum and count, the column's W^T y
            for (int h0 = 0; h0 < H; h0 += HC) {
                const int nh = H - h0 < HC ? H - h0 : HC;
                harm_wave_sync();
                for (int j = lane; j < nh; j += 64) row[j] = y[h0 + j];
                harm_wave_sync();
                // (selects, not branches: the loop unrolls and its LDS reads go out ahead of the chain of adds)
#pragma unroll 4
                for (int j = sg; j < nh; j += SG) {
                    const double v = row[j];
                    const bool ob = (int)s_site[h0 + j] == my_site && (!missing || v == v);
                    sum += ob ? v : 0.0;
                    n_i += ob ? 1 : 0;
                }
                if (my_q < Qp) {
#pragma unroll 4
                    for (int j = qg; j < nh; j += 64 / HQ) dacc += Wp[(h0 + j) * Qp + my_q] * row[j];
                }
            }
            for (int o = Bp; o < 64; o <<= 1) {          // the groups of a site, in a fixed order
                sum += __shfl_xor(sum, o, 64);
                n_i += __shfl_xor(n_i, o, 64);
            }
#pragma unroll
            for (int o = HQ; o < 64; o <<= 1) dacc += __shfl_xor(dacc, o, 64);
            harm_wave_sync();
            if (lane < HB) s_ybar[wv][lane] = (lane < B && n_i >= 1) ? sum / (double)n_i : 0.0;
            if (lane < HQ) s_d[wv][lane] = lane < Qp ? dacc : 0.0;
            harm_wave_sync();
            double d[HQ];
#pragma unroll
            for (int q = 0; q < HQ; ++q) d[q] = s_d[wv][q];
            // the residuals (lanes over the controls), then the site's sum of their squares (lane = site)
            for (int h0 = 0; h0 < H; h0 += HC) {
                const int nh = H - h0 < HC ? H - h0 : HC;
                if (H > HC) {            // (a row of one chunk is still there)
                    harm_wave_sync();
                    for (int j = lane; j < nh; j += 64) row[j] = y[h0 + j];
                }
                harm_wave_sync();
                for (int j = lane; j < nh; j += 64) {
                    const double v = row[j];
                    double fit = 0.0;
#pragma unroll
                    for (int q = 0; q < HQ; ++q)
                        if (q < Qp) fit += d[q] * Wp[(h0 + j) * Qp + q];
                    const double e = (v - s_ybar[wv][s_site[h0 + j]]) - fit;
                    row[j] = (missing && !(v == v)) ? 0.0 : e * e;
                }
                harm_wave_sync();
#pragma unroll 4
                for (int j = sg; j < nh; j += SG) sse_i += (int)s_site[h0 + j] == my_site ? row[j] : 0.0;
            }
            for (int o = Bp; o < 64; o <<= 1) sse_i += __shfl_xor(sse_i, o, 64);
        }
        const bool site = lane < B;
        int n = site ? n_i : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        const int Bc = __popcll(__ballot(site && n_i >= 1));
        const double sse = fcd_wave_sum(site && n_i >= 1 ? sse_i : 0.0);
        int status = ST_FITTED;
        if (bad) status = ST_SITE;
        else if (n - Bc - Qp < 1) status = ST_DOF;
        else if (!(sse == sse)) status = ST_NAN;
        else if (!(sse > 0.0)) status = ST_CONSTANT;
        const bool fitted = status == ST_FITTED;
        // beta = T d, by lane q; every lane then reads all of it
        double bq = nan;
        if (fitted && lane < Q) {
            bq = 0.0;
            for (int j = 0; j < Qp; ++j) bq += a.T[lane * Qp + j] * s_d[wv][j];
        }
        if (lane < HQ) s_beta[wv][lane] = (fitted && lane < Q) ? bq : 0.0;
        harm_wave_sync();
        double gm = nan, sd = nan, gh = nan, dh = nan;
        if (fitted) {
            const double sigma2 = sse / (double)n, sigma = sqrt(sigma2);
            double alpha = 0.0, wgt = 0.0;
            if (site && n_i >= 1) {
                double dot = 0.0;
                for (int q = 0; q < Q; ++q) dot += a.M[lane * Q + q] * s_beta[wv][q];
                alpha = s_ybar[wv][lane] - dot;
                wgt = ((double)n_i / (double)n) * alpha;
            }
            const double abar = fcd_wave_sum(wgt);
            gm = abar;
            sd = sigma;
            if (site && n_i >= 1) gh = (alpha - abar) / sigma;
            if (site && n_i >= 2) dh = sse_i / (sigma2 * (double)(n_i - 1));
        }
        if (site) {
            a.gamma_hat[(int64_t)lane * a.C + c] = gh;
            a.delta2_hat[(int64_t)lane * a.C + c] = dh;
            a.n_obs[(int64_t)lane * a.C + c] = n_i;
        }
        if (lane < Q) a.beta[c * Q + lane] = bq;
        if (lane == 0) {
            a.grand_mean[c] = gm;
            a.pooled_sd[c] = sd;
            a.info[c * 4 + 0] = n;
            a.info[c * 4 + 1] = Bc;
            a.info[c * 4 + 2] = Qp;
            a.info[c * 4 + 3] = status;
        }
    }
}

// ---- priors -----------------------------------------------------------------------------------------------------------
constexpr int PT = 1024;
__device__ __forceinline__ double harm_block_sum(double v, double *red) {       // a fixed tree over the 1024 threads
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int o = PT / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    return red[0];
}

// prior (6, B): gamma_bar, tau2, m, s2, a, b.  prior_info (B, 3): members of the gamma set, of the delta set, 1 = defined.
// Two passes over the site's two planes: counts and sums, then the centred squares; thread t takes connections t, t + 1024, ...
__global__ __launch_bounds__(PT) void harm_prior_kernel(const double *__restrict__ gamma_hat, const double *__restrict__ delta2_hat,
                                                        int64_t C, int B, int no_eb, double *__restrict__ prior,
                                                        int32_t *__restrict__ prior_info) {
    __shared__ double red[PT];
    const int i = blockIdx.x, t = threadIdx.x;
    const double nan = __builtin_nan("");
    double out[6] = {nan, nan, nan, nan, nan, nan};
    int cnt[2] = {0, 0};
    if (!no_eb) {
        const double *__restrict__ pg = gamma_hat + (int64_t)i * C;
        const double *__restrict__ pd = delta2_hat + (int64_t)i * C;
        double s[2] = {0.0, 0.0}, m[2] = {0.0, 0.0}, q[2] = {0.0, 0.0}, mean[2];
#pragma unroll 4
        for (int64_t c = t; c < C; c += PT) {
            const double g = pg[c], d = pd[c];
            s[0] += g == g ? g : 0.0;
            m[0] += g == g ? 1.0 : 0.0;
            s[1] += d == d ? d : 0.0;
            m[1] += d == d ? 1.0 : 0.0;
        }
        for (int k = 0; k < 2; ++k) {
            m[k] = harm_block_sum(m[k], red);
            mean[k] = harm_block_sum(s[k], red) / m[k];
        }
#pragma unroll 4
        for (int64_t c = t; c < C; c += PT) {
            const double g = pg[c], d = pd[c];
            q[0] += g == g ? (g - mean[0]) * (g - mean[0]) : 0.0;
            q[1] += d == d ? (d - mean[1]) * (d - mean[1]) : 0.0;
        }
        for (int k = 0; k < 2; ++k) {
            const double var = harm_block_sum(q[k], red) / (m[k] - 1.0);
            cnt[k] = (int)m[k];
            if (cnt[k] >= 1) out[2 * k] = mean[k];
            if (cnt[k] >= 2) out[2 * k + 1] = var;
        }
    }
    const double tau2 = out[1], m = out[2], s2 = out[3];
    const bool defined = !no_eb && cnt[0] >= 2 && cnt[1] >= 2 && tau2 > 0.0 && tau2 <= DBL_MAX && s2 > 0.0 && s2 <= DBL_MAX;
    if (defined) {
        out[4] = (2.0 * s2 + m * m) / s2;
        out[5] = (m * s2 + m * m * m) / s2;
    }
    if (t == 0) {
        for (int k = 0; k < 6; ++k) prior[k * B + i] = out[k];
        prior_info[i * 3 + 0] = cnt[0];
        prior_info[i * 3 + 1] = cnt[1];
        prior_info[i * 3 + 2] = defined ? 1 : 0;
    }
}

// ---- empirical Bayes ----------------------------------------------------------------------------------------------------
struct harm_eb_args {
    const double *gamma_hat, *delta2_hat, *pooled_sd, *prior;
    const int32_t *n_obs, *info, *prior_info;
    int64_t C;
    int B, no_eb;
    double *gamma_star, *delta2_star, *shift, *scale;
    int32_t *n_iter;
};

__global__ __launch_bounds__(256) void harm_eb_kernel(const harm_eb_args a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)a.B * a.C) return;
    const int i = (int)(e / a.C);
    const int64_t c = e % a.C;
    const double nan = __builtin_nan("");
    double gs = nan, ds = nan, shift = 0.0, scale = 1.0;
    int steps = 0;
    const bool fitted = a.info[c * 4 + 3] == ST_FITTED;
    const int n_i = a.n_obs[e];
    const double gh = a.gamma_hat[e], dh = a.delta2_hat[e];
    bool harmonised = false;
    if (fitted && a.no_eb) {
        gs = gh;
        ds = dh;
        harmonised = n_i >= 2 && dh > 0.0;
    } else if (fitted && a.prior_info[i * 3 + 2]) {
        const double gbar = a.prior[0 * a.B + i], tau2 = a.prior[1 * a.B + i], pa = a.prior[4 * a.B + i], pb = a.prior[5 * a.B + i];
        if (n_i == 0) {
            gs = gbar;
            ds = pb / (pa - 1.0);
        } else {
            const double nn = (double)n_i;
            const double ss = n_i >= 2 ? (nn - 1.0) * dh : 0.0;       // (n_i - 1) delta2_hat; 0 for a lone control
            double g = gh, d2 = n_i >= 2 ? dh : pb / (pa - 1.0);
            bool done = false;
            while (steps < EB_MAX_STEPS && !done) {
                const double g1 = (nn * tau2 * gh + d2 * gbar) / (nn * tau2 + d2);
                const double dev = gh - g1;
                const double d1 = (0.5 * (ss + nn * (dev * dev)) + pb) / (nn / 2.0 + pa - 1.0);
                done = fabs(g1 - g) <= EB_TOL * (1.0 + fabs(g1)) && fabs(d1 - d2) <= EB_TOL * d1;
                g = g1;
                d2 = d1;
                ++steps;
            }
            gs = g;
            ds = d2;
            if (!done) steps = -steps;          // the cap was hit: flagged by the sign
        }
        harmonised = true;
    }
    if (harmonised) {
        shift = a.pooled_sd[c] * gs;
        scale = sqrt(ds);
    }
    a.gamma_star[e] = gs;
    a.delta2_star[e] = ds;
    a.shift[e] = shift;
    a.scale[e] = scale;
    a.n_iter[e] = steps;
}

// ---- apply --------------------------------------------------------------------------------------------------------------
struct harm_zref {
    double v[HQ];
};
// grid = (blocks of AR rows, blocks of AS columns).  VEC: S is even and x / out are 16-byte aligned, a lane takes two columns.
constexpr int AR = 32, AS = 256;
template <bool VEC>
__global__ __launch_bounds__(256) void harm_apply_kernel(const double *__restrict__ x, const unsigned char *__restrict__ site,
                                                         const double *__restrict__ z, const harm_zref z_ref,
                                                         const double *__restrict__ grand_mean, const double *__restrict__ beta,
                                                         const double *__restrict__ shift, const double *__restrict__ scale,
                                                         int64_t C, int64_t S, int B, int Q, double *__restrict__ out,
                                                         volatile unsigned *err) {
    __shared__ __attribute__((aligned(16))) double zc[HQ * AS];      // [q][column]: z - z_ref of this block's columns
    __shared__ double s_shift[HB * AR], s_scale[HB * AR];            // [site][row]
    __shared__ unsigned char s_site[AS];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.y * AS, c0 = (int64_t)blockIdx.x * AR;
    const int ns = (int)(S - s0 < AS ? S - s0 : AS);
    const int nr = (int)(C - c0 < AR ? C - c0 : AR);
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int e = tid; e < ns * Q; e += 256) {
        const int j = e / Q, q = e % Q;
        zc[q * AS + j] = z[(s0 + j) * Q + q] - z_ref.v[q];
    }
    if (tid < ns) {
        const unsigned char s = site[s0 + tid];
        s_site[tid] = s;
        if ((int)s >= B) s_bad = 1;
    }
    for (int e = tid; e < B * AR; e += 256) {
        const int i = e / AR, r = e % AR;
        if (r < nr) {
            s_shift[e] = shift[(int64_t)i * C + c0 + r];
            s_scale[e] = scale[(int64_t)i * C + c0 + r];
        }
    }
    __syncthreads();
    if (s_bad && blockIdx.x == 0 && tid == 0)
        __hip_atomic_store(const_cast<unsigned *>(err), FCD_DEV_ERR_HARM_SITE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    constexpr int W = VEC ? 2 : 1, TPR = AS / W, RPI = 256 / TPR;   // columns per lane, lanes per row, rows per iteration
    const int j = (tid % TPR) * W, rr = tid / TPR;
    if (j >= ns) return;
    int si[W];
#pragma unroll
    for (int t = 0; t < W; ++t) si[t] = s_site[j + t];
    for (int r = rr; r < nr; r += RPI) {
        const int64_t c = c0 + r;
        const double *bq = beta + c * Q;
        const double gm = grand_mean[c];
        double d[W];
#pragma unroll
        for (int t = 0; t < W; ++t) d[t] = 0.0;
        for (int q = 0; q < Q; ++q) {
            const double bv = bq[q];
#pragma unroll
            for (int t = 0; t < W; ++t) d[t] = d[t] + bv * zc[q * AS + j + t];
        }
        const int64_t at = c * S + s0 + j;
        double xv[W], ov[W];
        if (VEC) {
            const double2 v = *reinterpret_cast<const double2 *>(x + at);      // (ns is even: j + 1 < ns)
            xv[0] = v.x;
            xv[W - 1] = v.y;
        } else {
            xv[0] = x[at];
        }
#pragma unroll
        for (int t = 0; t < W; ++t) {
            if (si[t] >= B) {
                ov[t] = __builtin_nan("");
            } else {
                const double sh = s_shift[si[t] * AR + r], sc = s_scale[si[t] * AR + r];
                const double m = gm + d[t];
                ov[t] = (sh == 0.0 && sc == 1.0) ? xv[t] : ((xv[t] - m) - sh) / sc + m;
            }
        }
        if (VEC)
            *reinterpret_cast<double2 *>(out + at) = make_double2(ov[0], ov[W - 1]);
        else
            out[at] = ov[0];
    }
}

const unsigned HARM_FLAGS = FCD_DATA_NAN_MISSING | FCD_HARMONIZE_NO_EB;

// the descriptor's head, common to both entry points
int harm_check(fcd_ctx *ctx, const fcd_harmonize_desc *d, const char *who) {
    if (!ctx || !d) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    if (d->size != sizeof(fcd_harmonize_desc))
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "descriptor of %lld bytes, this library knows %lld", (long long)d->size,
                            (long long)sizeof(fcd_harmonize_desc));
    if (d->flags & ~HARM_FLAGS) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "unknown flags 0x%llx", (long long)d->flags);
    if (d->C < 1 || d->B < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "C=%lld B=%lld must be >= 1", d->C, d->B);
    if (d->Q < 0 || d->Qp < 0 || d->Qp > d->Q) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "need 0 <= Qp <= Q (Q=%lld, Qp=%lld)", d->Q, d->Qp);
    if (d->B > HB) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "B=%lld sites, at most 64", d->B);
    if (d->Q > HQ) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "Q=%lld covariate columns, at most 8", d->Q);
    return FCD_OK;
}

}  // namespace

extern "C" int fcd_site_harmonize_fit(fcd_ctx *ctx, const fcd_harmonize_desc *d) {
    static const char *who = "fcd_site_harmonize_fit";
    int rc = harm_check(ctx, d, who);
    if (rc) return rc;
    if (d->H < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "H=%lld must be >= 1", d->H);
    if (d->H > HH) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "H=%lld controls, at most 4096", d->H);
    if (!d->b || !d->site || !d->grand_mean || !d->pooled_sd || !d->gamma_hat || !d->delta2_hat || !d->gamma_star ||
        !d->delta2_star || !d->shift || !d->scale || !d->n_obs || !d->n_iter || !d->info || !d->prior || !d->prior_info)
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    if (d->Q > 0 && (!d->beta || !d->z_bar || !d->z_ref)) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "Q=%lld but beta, z_bar or z_ref is null", d->Q);
    if (d->Qp > 0 && (!d->W || !d->T)) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "Qp=%lld but W or T is null", d->Qp);
    if (d->Qp > 0 && (d->flags & FCD_DATA_NAN_MISSING))
        return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "covariates with FCD_DATA_NAN_MISSING: every connection would need its own design");
    if (d->C > ((int64_t)1 << 40) / HB) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "shape too large (C=%lld)", d->C);
    hipStream_t st = (hipStream_t)d->stream;
    const int Q = (int)d->Q, Qp = (int)d->Qp, B = (int)d->B;
    // workspace: T (Q, Qp) | zbar - z_ref (B, Q); nothing of it outlives the call
    const int nT = Q * Qp, nM = B * Q;
    rc = fcd_ws_reserve(ctx, (size_t)(HQ * HQ + HB * HQ) * sizeof(double));
    if (rc) return rc;
    double *wsT = (double *)ctx->ws.p, *wsM = wsT + HQ * HQ;
    if (nT + nM > 0) {
        double host[HQ * HQ + HB * HQ];
        for (int e = 0; e < nT; ++e) host[e] = d->T[e];
        for (int e = 0; e < nM; ++e) host[HQ * HQ + e] = d->z_bar[e] - d->z_ref[e % Q];
        const int from[2] = {0, HQ * HQ}, count[2] = {nT, nM};
        for (int k = 0; k < 2; ++k) {
            for (int o = 0; o < count[k]; o += 128) {
                harm_chunk ch;
                const int m = count[k] - o < 128 ? count[k] - o : 128;
                for (int e = 0; e < 128; ++e) ch.v[e] = e < m ? host[from[k] + o + e] : 0.0;
                hipLaunchKernelGGL(harm_upload_kernel, dim3(1), dim3(128), 0, st, ch, wsT + from[k] + o, m);
                FCD_LAUNCH_CHECK();
            }
        }
    }
    harm_fit_args fa;
    fa.b = d->b;
    fa.site = d->site;
    fa.W = d->W;
    fa.T = wsT;
    fa.M = wsM;
    fa.C = d->C;
    fa.H = (int)d->H;
    fa.B = B;
    fa.Q = Q;
    fa.Qp = Qp;
    fa.missing = (d->flags & FCD_DATA_NAN_MISSING) ? 1 : 0;
    fa.grand_mean = d->grand_mean;
    fa.pooled_sd = d->pooled_sd;
    fa.beta = d->beta;
    fa.gamma_hat = d->gamma_hat;
    fa.delta2_hat = d->delta2_hat;
    fa.n_obs = d->n_obs;
    fa.info = d->info;
    fa.err = ctx->dev_err;
    const int64_t groups = (d->C + FIT_WAVES - 1) / FIT_WAVES, cap = (int64_t)ctx->num_cu * 8;
    hipLaunchKernelGGL(harm_fit_kernel, dim3((unsigned)(groups < cap ? groups : cap)), dim3(64 * FIT_WAVES), 0, st, fa);
    FCD_LAUNCH_CHECK();
    const int no_eb = (d->flags & FCD_HARMONIZE_NO_EB) ? 1 : 0;
    hipLaunchKernelGGL(harm_prior_kernel, dim3((unsigned)B), dim3(PT), 0, st, d->gamma_hat, d->delta2_hat, d->C, B, no_eb, d->prior,
                       d->prior_info);
    FCD_LAUNCH_CHECK();
    harm_eb_args ea;
    ea.gamma_hat = d->gamma_hat;
    ea.delta2_hat = d->delta2_hat;
    ea.pooled_sd = d->pooled_sd;
    ea.prior = d->prior;
    ea.n_obs = d->n_obs;
    ea.info = d->info;
    ea.prior_info = d->prior_info;
    ea.C = d->C;
    ea.B = B;
    ea.no_eb = no_eb;
    ea.gamma_star = d->gamma_star;
    ea.delta2_star = d->delta2_star;
    ea.shift = d->shift;
    ea.scale = d->scale;
    ea.n_iter = d->n_iter;
    hipLaunchKernelGGL(harm_eb_kernel, dim3((unsigned)((d->C * B + 255) / 256)), dim3(256), 0, st, ea);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}

extern "C" int fcd_site_harmonize_apply(fcd_ctx *ctx, const fcd_harmonize_desc *d) {
    static const char *who = "fcd_site_harmonize_apply";
    int rc = harm_check(ctx, d, who);
    if (rc) return rc;
    if (d->S < 1) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "S=%lld must be >= 1", d->S);
    if (!d->x || !d->out || !d->site || !d->grand_mean || !d->shift || !d->scale) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "null pointer");
    if (d->Q > 0 && (!d->z || !d->z_ref || !d->beta)) return fcd_fail_who(ctx, FCD_ERR_ARG, who, "Q=%lld but z, z_ref or beta is null", d->Q);
    const int64_t gx = (d->C + AR - 1) / AR, gy = (d->S + AS - 1) / AS;
    if (gx > INT32_MAX || gy > 65535) return fcd_fail_who(ctx, FCD_ERR_UNSUPPORTED, who, "shape too large (C=%lld, S=%lld)", d->C, d->S);
    hipStream_t st = (hipStream_t)d->stream;
    harm_zref zr;
    for (int q = 0; q < HQ; ++q) zr.v[q] = q < d->Q ? d->z_ref[q] : 0.0;
    const bool vec = (d->S % 2 == 0) && (((uintptr_t)d->x | (uintptr_t)d->out) % 16 == 0);
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (vec)
        hipLaunchKernelGGL(harm_apply_kernel<true>, grid, dim3(256), 0, st, d->x, d->site, d->z, zr, d->grand_mean, d->beta, d->shift,
                           d->scale, d->C, d->S, (int)d->B, (int)d->Q, d->out, ctx->dev_err);
    else
        hipLaunchKernelGGL(harm_apply_kernel<false>, grid, dim3(256), 0, st, d->x, d->site, d->z, zr, d->grand_mean, d->beta, d->shift,
                           d->scale, d->C, d->S, (int)d->B, (int)d->Q, d->out, ctx->dev_err);
    FCD_LAUNCH_CHECK();
    return FCD_OK;
}
