// Epipolar evaluation of match rows on the device -- reference utils/eval/measure.py:18-71 (sampson_distance,
// symmetric_epipolar_distance), networks/utils.py:74-110 (sym_epi_dist, sampson_dist) and the np.histogram of
// check_inliers_distr (measure.py:115-141): per row (x1, y1, x2, y2) of an item the distance to the epipolar geometry of the
// item's fundamental matrix, and per item the bin counts of those distances.  One work-group per item, like match_tail_kernel,
// whose outputs ([B,stride,4] float64 rows + device-side counts) are this kernel's natural input.  Compiled as part of
// filter.hip.
#pragma once
#include "host_pack.h"

// the emulator of the test-suite has no atomicAdd; an integer add is an integer add on either side
#ifndef P2P_ATOMIC_ADD_INT
#ifdef __HIPEMU__
#define P2P_ATOMIC_ADD_INT(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#else
#define P2P_ATOMIC_ADD_INT(p, v) atomicAdd((p), (v))
#endif
#endif

namespace p2p {

constexpr int EPI_MAX_BINS = 16;

struct EpiArgs {
    const void *matches;                      // [B][stride][4], in_dtype
    const int *counts;                        // [B]
    const double *F;                          // [B][9]
    const double *edges;                      // [nbins + 1] or null
    void *dist;                               // [B][stride], out_dtype
    int *hist;                                // [B][nbins] or null
    int stride, kind, nbins, in_dtype, out_dtype;
    double eps;
};

// The ONE arithmetic of the entry point (include/p2p_hip.h states it): fp64 throughout, every multiply-add an explicit fma,
// every other operation a single IEEE operation, in this order.  No expression here has the shape a * b + c, and contraction
// is switched off on top of that, so hipcc for gfx950 and clang for x86 evaluate the same sequence of roundings.
__device__ __forceinline__ double epi_distance(const double *f, double x1, double y1, double x2, double y2, int kind, double eps) {
#pragma clang fp contract(off)
    if (kind == P2P_EPI_VALUE) return x1;                       // a distance computed earlier: only stored and binned
    const double l20 = fma(f[0], x1, fma(f[1], y1, f[2]));      // l2 = F x1
    const double l21 = fma(f[3], x1, fma(f[4], y1, f[5]));
    const double l22 = fma(f[6], x1, fma(f[7], y1, f[8]));
    const double l10 = fma(f[0], x2, fma(f[3], y2, f[6]));      // l1 = F^T x2 (its third component is never used)
    const double l11 = fma(f[1], x2, fma(f[4], y2, f[7]));
    const double dd = fma(x2, l20, fma(y2, l21, l22));          // x2 . l2
    const double p1 = l10 * l10, p2 = l20 * l20;
    const double s1 = fma(l11, l11, p1), s2 = fma(l21, l21, p2);
    const double e1 = eps + s1;
    if (kind == P2P_EPI_SAMPSON) {
        const double den = e1 + s2, sq = dd * dd;
        return sq / den;
    }
    const double e2 = eps + s2;
    if (kind == P2P_EPI_SYM) {
        const double r1 = 1.0 / e1, r2 = 1.0 / e2, sq = dd * dd;
        const double r = r1 + r2;
        return sq * r;
    }
    const double r1 = 1.0 / sqrt(e1), r2 = 1.0 / sqrt(e2);
    const double r = r1 + r2;
    return fabs(dd) * r;
}

// np.histogram(values, edges)[0]: bin i is [e_i, e_i+1), the last bin also holds its right edge; values outside
// [e_0, e_nbins] and NaNs fall in no bin (-1)
__device__ __forceinline__ int epi_bin(const double *edge, int nbins, double v) {
    if (!(v >= edge[0] && v <= edge[nbins])) return -1;
    int bin = 0;
    for (int i = 1; i < nbins; ++i) bin += v >= edge[i];
    return bin;
}

// Thread t of the item's work-group takes rows t, t + FT, ...; a row's distance depends on the row and the item's F alone.
// Bin counts: integer LDS atomics into one sub-histogram per wave, added up by the first nbins threads -- integers, so any
// order gives the same counts.  The distance that is binned is the one that is stored (after the rounding to fp32 if any).
__global__ __launch_bounds__(FT) void epipolar_kernel(EpiArgs a) {
    __shared__ int whist[FT / 64][EPI_MAX_BINS];
    __shared__ double edge[EPI_MAX_BINS + 1];
    const int tid = threadIdx.x, item = blockIdx.x, wave = tid >> 6;
    const bool binned = a.hist != nullptr;
    if (binned) {
        if (tid < (FT / 64) * EPI_MAX_BINS) (&whist[0][0])[tid] = 0;
        if (tid <= a.nbins) edge[tid] = a.edges[tid];
        __syncthreads();
    }
    const int n = min(a.counts[item], a.stride);          // < 0: the item passes through, no row is touched
    double f[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = a.F[(size_t)item * 9 + i];
    const size_t base = (size_t)item * a.stride;
    for (int j = tid; j < n; j += FT) {
        const size_t r = (base + j) * 4;
        double x1, y1, x2, y2;
        if (a.in_dtype == P2P_F64) {
            const double *m = (const double *)a.matches + r;
            x1 = m[0]; y1 = m[1]; x2 = m[2]; y2 = m[3];
        } else if (a.in_dtype == P2P_F32) {
            const float *m = (const float *)a.matches + r;
            x1 = (double)m[0]; y1 = (double)m[1]; x2 = (double)m[2]; y2 = (double)m[3];
        } else {
            const long long *m = (const long long *)a.matches + r;
            x1 = (double)m[0]; y1 = (double)m[1]; x2 = (double)m[2]; y2 = (double)m[3];
        }
        double d = epi_distance(f, x1, y1, x2, y2, a.kind, a.eps);
        if (a.out_dtype == P2P_F64) {
            ((double *)a.dist)[base + j] = d;
        } else {
            const float d32 = (float)d;
            ((float *)a.dist)[base + j] = d32;
            d = (double)d32;
        }
        if (binned) {
            const int bin = epi_bin(edge, a.nbins, d);
            if (bin >= 0) P2P_ATOMIC_ADD_INT(&whist[wave][bin], 1);
        }
    }
    if (!binned) return;
    __syncthreads();
    if (tid < a.nbins) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < FT / 64; ++w) total += whist[w][tid];
        a.hist[(size_t)item * a.nbins + tid] = total;
    }
}

}  // namespace p2p

extern "C" int p2p_epipolar_batch(const void *matches, int matches_dtype, const int *counts, const double *F, int batch, int stride,
                                  int kind, double eps, const double *edges, int nbins, void *dist, int dist_dtype, int *hist,
                                  p2p_stream_t stream) {
    P2P_REQUIRE(matches && counts && F && dist, P2P_EINVAL, "p2p_epipolar: null argument");
    P2P_REQUIRE(batch >= 1 && batch <= 65535 && stride >= 1, P2P_EINVAL, "p2p_epipolar: bad sizes (batch %d, stride %d)", batch, stride);
    P2P_REQUIRE(matches_dtype == P2P_F32 || matches_dtype == P2P_F64 || matches_dtype == P2P_I64, P2P_EINVAL,
                "p2p_epipolar: unknown matches dtype %d", matches_dtype);
    P2P_REQUIRE(dist_dtype == P2P_F32 || dist_dtype == P2P_F64, P2P_EINVAL, "p2p_epipolar: unknown dist dtype %d", dist_dtype);
    P2P_REQUIRE(kind == P2P_EPI_SAMPSON || kind == P2P_EPI_SYM || kind == P2P_EPI_SYM_SQRT || kind == P2P_EPI_VALUE, P2P_EINVAL, "p2p_epipolar: unknown kind %d", kind);
    P2P_REQUIRE(eps >= 0.0, P2P_EINVAL, "p2p_epipolar: eps must be >= 0 and not NaN");
    P2P_REQUIRE((hist != nullptr) == (edges != nullptr), P2P_EINVAL, "p2p_epipolar: hist and edges go together");
    P2P_REQUIRE(hist ? nbins >= 1 : nbins == 0, P2P_EINVAL, "p2p_epipolar: nbins %d (>= 1 with a histogram, 0 without)", nbins);
    P2P_REQUIRE(nbins <= p2p::EPI_MAX_BINS, P2P_EUNSUPPORTED, "p2p_epipolar: %d bins (at most %d)", nbins, p2p::EPI_MAX_BINS);
    p2p::EpiArgs a{matches, counts, F, edges, dist, hist, stride, kind, nbins, matches_dtype, dist_dtype, eps};
    hipLaunchKernelGGL(p2p::epipolar_kernel, dim3(batch), dim3(p2p::FT), 0, (hipStream_t)stream, a);
    return p2p::check_launch("epipolar_kernel");
}
