// Coarse stage, match extraction (ncn/extract_ncmatches.py:6-94 twice; patch2pix.py:340-375) and its top-k form (:96-158): per
// cell of one image the best cell(s) of the other, relocalised and scaled to pixels, with the softmax (or raw) score.  One
// scan per direction, instantiated as the one-candidate kernels and as the top-k kernels.  Compiled as part of coarse.hip.
#pragma once
#include "coarse_common.h"

namespace p2p {

__device__ __forceinline__ MatchArgs match_args_of_pair(MatchArgs m, size_t z) {
    m.X += z * m.sX;
    if (m.delta) m.delta += z * m.sX;
    m.matches += z * m.sM * 4;
    m.scores += z * m.sM;
    return m;
}

// one match row: cell (ra, cb) relocalised and scaled to pixels; `s` is the softmax denominator of the row's maximum
// (RECIP) or the score itself (the top-k kernels)
template <bool RECIP>
__device__ __forceinline__ void emit_match_as(const MatchArgs &m, int out_row, int ra, int cb, float s) {
    int ia = ra / m.wA, ja = ra - ia * m.wA, ib = cb / m.wB, jb = cb - ib * m.wB;
    if (m.ksize > 1 && m.delta) {
        const int k = m.ksize;
        int code = m.delta[(size_t)ra * (m.hB * m.wB) + cb];
        const int dl = code % k; code /= k;
        const int dk = code % k; code /= k;
        const int dj = code % k; code /= k;
        ia = ia * k + code; ja = ja * k + dj; ib = ib * k + dk; jb = jb * k + dl;
    } else if (m.ksize > 1) {
        ia *= m.ksize; ja *= m.ksize; ib *= m.ksize; jb *= m.ksize;
    }
    const long long up = m.upsample, off = m.center ? m.upsample / 2 : 0;
    long long *o = m.matches + (size_t)out_row * 4;
    o[0] = up * ja + off; o[1] = up * ia + off; o[2] = up * jb + off; o[3] = up * ib + off;
    m.scores[out_row] = RECIP ? 1.0f / s : s;       // max of softmax = exp(0) / sum exp(x - max)
}
__device__ __forceinline__ void emit_match(const MatchArgs &m, int out_row, int ra, int cb, float sum_exp) { emit_match_as<true>(m, out_row, ra, cb, sum_exp); }

// The topk best cells per cell and direction (corr_to_matches_topk, extract_ncmatches.py:96-158), ordered by descending
// value and, among equal values, ascending index.  No candidate list is kept (indexed at run time it would live in
// scratch): rank t is the arg-max over the cells that come strictly AFTER rank t-1's (value, index) in that order, found
// by one more pass of the reduction over a volume that sits in L2 / Infinity Cache.  topk passes, plus the softmax sum
// after rank 0.  do_softmax = 0: the score is the value itself.
// ONE = the one-candidate kernels (topk and do_softmax are not read): every cell a candidate, the score 1 / sum exp, and the
// scan returns after rank 0 -- the filter, the do_softmax switch, the index clamp and the rank loop are not compiled.  Both
// forms are the same slices and the same tree, so rank 0 of topk = 1 with softmax is the one-candidate output bit for bit.
template <bool ONE>
__device__ __forceinline__ bool match_candidate(float v, int i, float pv, int pi) {      // (v, i) comes after (pv, pi)
    if constexpr (ONE) return true;
    else return v < pv || (v == pv && i > pi);
}

// direction B->A: one block per 16 columns (a row of the block = half a 128-byte line: 8-column blocks fetched every line of
// the volume four times; 32 columns leave too few blocks per pair), 16 interleaved row slices.
// Rank t of column c -> row t*nB + c (the reference's view(batch, topk, -1)).
constexpr int MC_COLS = 16, MC_SLICES = 16;
template <bool ONE>
__device__ __forceinline__ void match_cols_scan(const MatchArgs &m_, int topk, int do_softmax) {
    const MatchArgs m = match_args_of_pair(m_, blockIdx.z);
    __shared__ float smax[MC_SLICES][MC_COLS];
    __shared__ int sarg[MC_SLICES][MC_COLS];
    __shared__ float ssum[MC_SLICES][MC_COLS];
    const int nA = m.hA * m.wA, nB = m.hB * m.wB;
    const int cs = threadIdx.x & (MC_COLS - 1), rs = threadIdx.x / MC_COLS;
    const int col = blockIdx.x * MC_COLS + cs;
    const bool ok = col < nB;
    float pv = INFINITY, top = 0.f, total = 1.f;     // previous rank's value (everything comes after +inf, -1), rank 0's, sum exp
    int pi = -1;
    for (int t = 0; ONE || t < topk; ++t) {
        float best = -INFINITY;
        int arg = 0x7fffffff;
        if (ok)
            for (int r = rs; r < nA; r += MC_SLICES) {
                const float v = m.X[(size_t)r * nB + col];
                if (match_candidate<ONE>(v, r, pv, pi) && v > best) { best = v; arg = r; }
            }
        smax[rs][cs] = best; sarg[rs][cs] = arg;
        __syncthreads();
        float gb = smax[0][cs];
        int ga = sarg[0][cs];
#pragma unroll
        for (int s = 1; s < MC_SLICES; ++s) {
            const float v = smax[s][cs];
            const int a = sarg[s][cs];
            if (v > gb || (v == gb && a < ga)) { gb = v; ga = a; }
        }
        bool softmax = true;
        if constexpr (!ONE) softmax = do_softmax;
        if (t == 0) {
            top = gb;
            if (softmax) {
                float sum = 0.f;
                if (ok)
                    for (int r = rs; r < nA; r += MC_SLICES) sum += expf(m.X[(size_t)r * nB + col] - gb);
                ssum[rs][cs] = sum;
                __syncthreads();
                if (rs == 0 && ok) {
                    total = 0.f;
#pragma unroll
                    for (int s = 0; s < MC_SLICES; ++s) total += ssum[s][cs];
                }
            }
        }
        if constexpr (ONE) {
            if (rs == 0 && ok) emit_match(m, col, ga, col, total);
            return;
        } else {
            // topk <= nA finite values always leave a candidate; a volume of NaN / -inf does not, and must not index past the delta
            ga = min(ga, nA - 1);
            if (rs == 0 && ok)
                emit_match_as<false>(m, t * nB + col, ga, col, softmax ? (t == 0 ? 1.0f : expf(gb - top)) / total : gb);
            pv = gb; pi = ga;
            __syncthreads();        // the next rank overwrites smax / sarg
        }
    }
}
__global__ __launch_bounds__(256) void match_cols_kernel(MatchArgs m) { match_cols_scan<true>(m, 1, 1); }
__global__ __launch_bounds__(256) void match_cols_topk_kernel(MatchArgs m, int topk, int do_softmax) { match_cols_scan<false>(m, topk, do_softmax); }

// direction A->B: one wave per row.  Rank t of row r -> row topk*nB + r*topk + t (view(batch, -1, topk), after the whole
// B->A list).
template <bool ONE>
__device__ __forceinline__ void match_rows_scan(const MatchArgs &m_, int topk, int do_softmax) {
    const MatchArgs m = match_args_of_pair(m_, blockIdx.z);
    const int nA = m.hA * m.wA, nB = m.hB * m.wB;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= nA) return;
    const float *x = m.X + (size_t)row * nB;
    float pv = INFINITY, top = 0.f, total = 1.f;
    int pi = -1;
    for (int t = 0; ONE || t < topk; ++t) {
        float best = -INFINITY;
        int arg = 0x7fffffff;
        for (int c = lane; c < nB; c += 64) {
            const float v = x[c];
            if (match_candidate<ONE>(v, c, pv, pi) && v > best) { best = v; arg = c; }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const float ov = __shfl_xor(best, s);
            const int oa = __shfl_xor(arg, s);
            if (ov > best || (ov == best && oa < arg)) { best = ov; arg = oa; }
        }
        bool softmax = true;
        if constexpr (!ONE) softmax = do_softmax;
        if (t == 0) {
            top = best;
            if (softmax) {
                float sum = 0.f;
                for (int c = lane; c < nB; c += 64) sum += expf(x[c] - best);
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s);
                total = sum;
            }
        }
        if constexpr (ONE) {
            if (lane == 0) emit_match(m, nB + row, row, arg, total);
            return;
        } else {
            arg = min(arg, nB - 1);
            if (lane == 0)
                emit_match_as<false>(m, topk * nB + row * topk + t, row, arg, softmax ? (t == 0 ? 1.0f : expf(best - top)) / total : best);
            pv = best; pi = arg;
        }
    }
}
__global__ __launch_bounds__(256) void match_rows_kernel(MatchArgs m) { match_rows_scan<true>(m, 1, 1); }
__global__ __launch_bounds__(256) void match_rows_topk_kernel(MatchArgs m, int topk, int do_softmax) { match_rows_scan<false>(m, topk, do_softmax); }

void launch_matches(const MatchArgs &m, int batch, hipStream_t stream) {
    hipLaunchKernelGGL(match_cols_kernel, dim3(ceil_div(m.hB * m.wB, MC_COLS), 1, batch), dim3(256), 0, stream, m);
    hipLaunchKernelGGL(match_rows_kernel, dim3(ceil_div(m.hA * m.wA, 4), 1, batch), dim3(256), 0, stream, m);
}

void launch_matches_topk(const MatchArgs &m, int batch, int topk, int do_softmax, hipStream_t stream) {
    hipLaunchKernelGGL(match_cols_topk_kernel, dim3(ceil_div(m.hB * m.wB, MC_COLS), 1, batch), dim3(256), 0, stream, m, topk, do_softmax);
    hipLaunchKernelGGL(match_rows_topk_kernel, dim3(ceil_div(m.hA * m.wA, 4), 1, batch), dim3(256), 0, stream, m, topk, do_softmax);
}

__global__ void delta_unpack_kernel(const uint8_t *__restrict__ delta, size_t n, int k, long long *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int s = delta[i];
    out[3 * n + i] = s % k; s /= k;
    out[2 * n + i] = s % k; s /= k;
    out[1 * n + i] = s % k; s /= k;
    out[i] = s;
}

void launch_delta_unpack(const uint8_t *delta, size_t n, int k, long long *out, hipStream_t stream) {
    hipLaunchKernelGGL(delta_unpack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, delta, n, k, out);
}

}  // namespace p2p
