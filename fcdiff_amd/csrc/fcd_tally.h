// What the post-fit tallies over the sampler's r_bits share (fcd_count.hip, fcd_region_sets.hip, fcd_patient_groups.hip,
// fcd_patient_traits.hip; fcd_coanomaly.hip takes tally_q alone): the bit-sliced counters, the "bin a row in LDS, add it
// in place" histogram step, the staged row of r words, q from lq_R, and on the host the checks, the device tables and the
// scratch they all size the same way.  The first part is plain C++: tests/tally_check.cpp drives it under g++.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/fcdiff_hip.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define FCD_TALLY_HD __host__ __device__ __forceinline__
#else
#define FCD_TALLY_HD inline
#endif

// Bit-sliced (vertical) counters of 64 chains: bit c of pl[b] is bit b of chain c's count, so adding a word of 64 chain
// bits is one carry-save step over the planes.  Counts up to 2^P - 1; a carry out of the top plane is dropped (the callers
// bound what they add).
template <int P>
struct tally_planes {
    typedef uint64_t __attribute__((may_alias)) word4;      // four uint16 counts, stored together
    uint64_t pl[P];
    FCD_TALLY_HD void clear() {
#pragma unroll
        for (int b = 0; b < P; ++b) pl[b] = 0;
    }
    FCD_TALLY_HD void add(uint64_t carry) {
#pragma unroll
        for (int b = 0; b < P; ++b) {
            const uint64_t t = pl[b] & carry;
            pl[b] ^= carry;
            carry = t;
        }
    }
    // bit c: chain c's count is not 0
    FCD_TALLY_HD uint64_t any() const {
        uint64_t a = 0;
#pragma unroll
        for (int b = 0; b < P; ++b) a |= pl[b];
        return a;
    }
    // chain c's count to row[c], c = 0 .. 63, four per 8-byte store (row: 8-byte aligned).  One shift per plane brings the
    // bits of four chains down, taken from a 32-bit half of the plane: the same walk over whole 64-bit planes keeps twice
    // the registers in flight, which put region_set_sums_kernel past 64 VGPRs (8 waves per SIMD).  Both sums kernels sit
    // just under that line; after a change here read their resource remarks and the LDS reads of count_sums_kernel's
    // region role (four in flight), and time the tallies (profiles/tally_family_cost.json).
    FCD_TALLY_HD void store16(uint16_t *row) const {
        word4 *dst = reinterpret_cast<word4 *>(row);
        for (int h = 0; h < 2; ++h) {                    // chains 0 .. 31 from the low halves of the planes, then the high ones
            uint32_t w[P];
#pragma unroll
            for (int b = 0; b < P; ++b) w[b] = (uint32_t)(pl[b] >> (32 * h));
            for (int c0 = 0; c0 < 32; c0 += 4) {
                uint32_t lo = 0, hi = 0;                 // counts of chains c0, c0 + 1 | c0 + 2, c0 + 3 of this half
#pragma unroll
                for (int b = 0; b < P; ++b) {
                    const uint32_t t = w[b] >> c0;       // bits 0 .. 3: bit b of the four counts
                    lo |= ((t & 1u) | (t & 2u) << 15) << b;
                    hi |= ((t >> 2 & 1u) | (t >> 2 & 2u) << 15) << b;
                }
                *dst++ = (uint64_t)hi << 32 | lo;
            }
        }
    }
};

// The checks on J index lists in CSR form (region sets, patient groups), `noun` being "set" or "group": offsets[0] = 0, no
// empty list, members non-negative and increasing inside a list.  A refusal goes through fail(code, format, a, b), whose
// result is returned; else FCD_OK with the largest size and the largest member.  With these an index below *max_member + 1
// elements and a count below *smax + 1 bins are in range, which is what lets the kernels read the lists unchecked.
template <typename FAIL>
int tally_csr_check(FAIL fail, const char *noun, const int32_t *offsets, const int32_t *members, int64_t J, int64_t *smax,
                    int64_t *max_member) {
    char fmt[96];
    *smax = 0;
    *max_member = -1;
    if (offsets[0] != 0) return fail(FCD_ERR_ARG, "offsets[0]=%lld", offsets[0], 0);
    for (int64_t j = 0; j < J; ++j) {
        const int64_t i0 = offsets[j], size = (int64_t)offsets[j + 1] - i0;
        if (size < 1) {
            snprintf(fmt, sizeof(fmt), "%s %%lld is empty", noun);
            return fail(FCD_ERR_ARG, fmt, j, 0);
        }
        for (int64_t i = i0; i < i0 + size; ++i) {
            const int64_t n = members[i];
            if (n < 0) {
                snprintf(fmt, sizeof(fmt), "%s %%lld has the negative member %%lld", noun);
                return fail(FCD_ERR_ARG, fmt, j, n);
            }
            if (i > i0 && n <= members[i - 1]) {
                snprintf(fmt, sizeof(fmt), "the members of %s %%lld do not increase at %%lld", noun);
                return fail(FCD_ERR_ARG, fmt, j, n);
            }
            if (n > *max_member) *max_member = n;
        }
        if (size > *smax) *smax = size;
    }
    return FCD_OK;
}

#ifdef __HIPCC__
#include "fcd_common.h"

// ---------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------

// One histogram row per workgroup: the row's per-chain counts are binned with LDS atomics, then the bins are added to the
// row in place.  The row belongs to this workgroup alone, so no global atomics (same-address device-scope atomics from every
// chain word cost ~70 us per tally at cfg3 in the first form of count_hist_kernel).  The two halves, for the kernels that
// bin by a rule of their own between them (a barrier after each):
__device__ __forceinline__ void tally_bins_clear(uint32_t *bins, int nb) {
    for (int k = threadIdx.x; k < nb; k += blockDim.x) bins[k] = 0;
}
// (bins that stayed 0 leave their words of out untouched)
__device__ __forceinline__ void tally_bins_flush(const uint32_t *bins, int nb, uint32_t *__restrict__ out) {
    for (int k = threadIdx.x; k < nb; k += blockDim.x) {
        const uint32_t c = bins[k];
        if (c) out[k] += c;
    }
}
// ... and the whole row: out[k] += #{g < G : min(src[g], L) = k}, k = 0 .. L.  Only the chains g < G are binned.
__device__ __forceinline__ void tally_bin_row(const uint16_t *__restrict__ src, int64_t G, int L, uint32_t *bins,
                                              uint32_t *__restrict__ out) {
    tally_bins_clear(bins, L + 1);
    __syncthreads();
    for (int64_t g = threadIdx.x; g < G; g += blockDim.x) atomicAdd(&bins[min((int)src[g], L)], 1u);
    __syncthreads();
    tally_bins_flush(bins, L + 1, out);
}

// Row rho of one chain word (rw = r_bits + w Nreg U) into LDS, all THREADS threads: roww[t] = the word of region rho and
// patient t for rho < Nreg, the OR over the members of region set rho - Nreg else (coalesced over t), and ZERO for
// U <= t < 64 ceil(U/64): the callers walk past U (whole 64-patient chunks, or U rounded up to 8), never into stale LDS.
template <int THREADS>
__device__ __forceinline__ void tally_stage_row(const uint64_t *__restrict__ rw, const int32_t *__restrict__ rs_offsets,
                                                const int32_t *__restrict__ rs_members, int rho, int Nreg, int U,
                                                uint64_t *roww) {
    const int NC = (U + 63) / 64;
    for (int t = threadIdx.x; t < NC * 64; t += THREADS) {
        uint64_t v = 0;
        if (t < U) {
            if (rho < Nreg) {
                v = rw[(int64_t)rho * U + t];
            } else {
                const int i0 = rs_offsets[rho - Nreg], i1 = rs_offsets[rho - Nreg + 1];
                for (int i = i0; i < i1; ++i) v |= rw[(int64_t)rs_members[i] * U + t];
            }
        }
        roww[t] = v;
    }
}

// q0 = P(r = 0), q1 = P(r = 1) of one site from lq_R, normalised in log space (the larger log-weight subtracted), so lq_R
// need not be normalised and q = 0 / q = 1 come out exact
__device__ __forceinline__ void tally_q(const double *__restrict__ lq_R, int64_t site, double &q0, double &q1) {
    const double l0 = lq_R[site * 2], l1 = lq_R[site * 2 + 1];
    const double mx = fmax(l0, l1);
    const double e0 = exp(l0 - mx), e1 = exp(l1 - mx);
    const double s = e0 + e1;
    q0 = e0 / s;
    q1 = e1 / s;
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------

// rows of a tally over patients: the regions, then (with_rs) the context's region sets
static inline int64_t tally_rows(const fcd_ctx *ctx, int64_t Nreg, int with_rs) { return Nreg + (with_rs ? ctx->rs_J : 0); }

// ... and what such a tally refuses about them; `what` = "groups" or "traits", the things that were set with_rs
static inline int tally_set_rows_check(fcd_ctx *ctx, int64_t Nreg, int with_rs, const char *who, const char *what) {
    if (!with_rs) return FCD_OK;
    if (ctx->rs_J < 1) {
        char text[96];
        snprintf(text, sizeof(text), "the %s were set with region sets and there are none", what);
        return fcd_fail_who(ctx, FCD_ERR_ARG, who, text);
    }
    if (ctx->rs_max_member >= Nreg)
        return fcd_fail_who(ctx, FCD_ERR_SHAPE, who, "member %lld of a region set with Nreg=%lld", ctx->rs_max_member, Nreg);
    return FCD_OK;
}

// Replace a device table the context owns (*slot) by a copy of the host pieces a | b (b may be empty; both empty: no
// table).  Nothing changes if the copy fails; freeing the old table waits for the tallies that read it.
static inline int tally_table_replace(fcd_ctx *ctx, void **slot, const void *a, size_t na, const void *b = nullptr, size_t nb = 0) {
    void *dev = nullptr;
    if (na + nb) {
        FCD_HIP_TRY(hipMalloc(&dev, na + nb));
        ctx->n_alloc += 1;
        hipError_t e = hipMemcpy(dev, a, na, hipMemcpyHostToDevice);
        if (e == hipSuccess && nb) e = hipMemcpy((char *)dev + na, b, nb, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(dev);
            return (int)e;
        }
    }
    if (*slot) (void)hipFree(*slot);
    *slot = dev;
    return FCD_OK;
}

// The scratch of a tally, `rows` rows of 64 ceil(G/64) per-chain counts of `bytes_per_count` each: the count tallies run one
// after another on one stream and share fcd_ctx::count_ws.  Above 1 GiB it is refused with `refusal` (a, b), where there is one.
static inline int tally_ws_reserve(fcd_ctx *ctx, int64_t rows, int64_t G, size_t bytes_per_count, const char *refusal = nullptr,
                                   long long a = 0, long long b = 0) {
    const size_t bytes = (size_t)rows * (size_t)((G + 63) / 64) * 64 * bytes_per_count;
    if (refusal && bytes > ((size_t)1 << 30)) return fcd_fail(ctx, FCD_ERR_UNSUPPORTED, refusal, a, b);
    return fcd_buf_reserve(ctx, ctx->count_ws, bytes);
}

// grid of a grid-stride tally launch: eight workgroups per CU at the most
static inline unsigned tally_grid(const fcd_ctx *ctx, int64_t blocks) {
    const int64_t cap = (int64_t)ctx->num_cu * 8;
    return (unsigned)(blocks < cap ? blocks : cap);
}
#endif
