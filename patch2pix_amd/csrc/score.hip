// Coarse stage, pair score (Patch2Pix.cal_coarse_score, patch2pix.py:320-338): per cell of either image the best normalised
// consensus value over the cells of the other image, and per pair the mean of those nA + nB cell scores.  The scans are the
// slices and trees of matches.hip (16 interleaved row slices per block of 16 columns; one wave per row), so a softmax cell
// score is the score the one-candidate match kernels give that cell, bit for bit.  Compiled as part of coarse.hip.
#pragma once
#include "matches.hip"

namespace p2p {

// NORM: P2P_SCORE_NONE the maximum itself; P2P_SCORE_SOFTMAX 1 / sum exp(x - max); P2P_SCORE_L1 max(x / (sum x + 1e-4)) =
// max(x) / d for d = sum x + 1e-4 > 0 and min(x) / d for d < 0 (a correctly rounded division is monotone): maximum, minimum
// and sum from ONE scan, one division.  One launch for both directions: the first col_groups work-groups take 16 columns
// each (cells[nA + c], the B cells), the others four rows each (cells[r], the A cells) -- the order of the reference's
// torch.cat([scores_A, scores_B]).
constexpr float SCORE_L1_EPS = 0.0001f;
template <int NORM>
__global__ __launch_bounds__(256) void score_cells_kernel(ScoreArgs a, int col_groups) {
    __shared__ float smax[MC_SLICES][MC_COLS];
    __shared__ float smin[MC_SLICES][MC_COLS];
    __shared__ float ssum[MC_SLICES][MC_COLS];
    const int nA = a.nA, nB = a.nB;
    const float *X = a.X + blockIdx.z * a.sX;
    float *cells = a.cells + blockIdx.z * ((size_t)nA + nB);
    if ((int)blockIdx.x < col_groups) {
        const int cs = threadIdx.x & (MC_COLS - 1), rs = threadIdx.x / MC_COLS;
        const int col = blockIdx.x * MC_COLS + cs;
        const bool ok = col < nB;
        float best = -INFINITY, low = INFINITY, sum = 0.f;
        if (ok)
            for (int r = rs; r < nA; r += MC_SLICES) {
                const float v = X[(size_t)r * nB + col];
                if (v > best) best = v;
                if constexpr (NORM == P2P_SCORE_L1) {
                    if (v < low) low = v;
                    sum += v;
                }
            }
        smax[rs][cs] = best;
        if constexpr (NORM == P2P_SCORE_L1) { smin[rs][cs] = low; ssum[rs][cs] = sum; }
        __syncthreads();
        float gb = smax[0][cs];
#pragma unroll
        for (int s = 1; s < MC_SLICES; ++s) {
            const float v = smax[s][cs];
            if (v > gb) gb = v;
        }
        if constexpr (NORM == P2P_SCORE_SOFTMAX) {
            sum = 0.f;
            if (ok)
                for (int r = rs; r < nA; r += MC_SLICES) sum += expf(X[(size_t)r * nB + col] - gb);
            ssum[rs][cs] = sum;
            __syncthreads();
        }
        if (rs != 0 || !ok) return;
        float total = 0.f, gl = INFINITY;
        if constexpr (NORM != P2P_SCORE_NONE) {
#pragma unroll
            for (int s = 0; s < MC_SLICES; ++s) total += ssum[s][cs];
        }
        if constexpr (NORM == P2P_SCORE_L1) {
#pragma unroll
            for (int s = 0; s < MC_SLICES; ++s) {
                const float v = smin[s][cs];
                if (v < gl) gl = v;
            }
            const float d = total + SCORE_L1_EPS;
            cells[nA + col] = (d < 0.f ? gl : gb) / d;
        } else {
            cells[nA + col] = NORM == P2P_SCORE_SOFTMAX ? 1.0f / total : gb;      // max of softmax = exp(0) / sum exp(x - max)
        }
        return;
    }
    const int row = ((int)blockIdx.x - col_groups) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= nA) return;
    const float *x = X + (size_t)row * nB;
    float best = -INFINITY, low = INFINITY, sum = 0.f;
    for (int c = lane; c < nB; c += 64) {
        const float v = x[c];
        if (v > best) best = v;
        if constexpr (NORM == P2P_SCORE_L1) {
            if (v < low) low = v;
            sum += v;
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const float ov = __shfl_xor(best, s);
        if (ov > best) best = ov;
        if constexpr (NORM == P2P_SCORE_L1) {
            const float ol = __shfl_xor(low, s);
            if (ol < low) low = ol;
            sum += __shfl_xor(sum, s);
        }
    }
    if constexpr (NORM == P2P_SCORE_SOFTMAX) {
        for (int c = lane; c < nB; c += 64) sum += expf(x[c] - best);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s);
    }
    if (lane != 0) return;
    if constexpr (NORM == P2P_SCORE_L1) {
        const float d = sum + SCORE_L1_EPS;
        cells[row] = (d < 0.f ? low : best) / d;
    } else {
        cells[row] = NORM == P2P_SCORE_SOFTMAX ? 1.0f / sum : best;
    }
}

// pair[z] = mean of the pair's nA + nB cell scores.  One work-group per pair whatever the batch: thread t adds the cells
// t, t + 256, ... in ascending order, a wave adds its 64 partial sums in an xor tree, thread 0 the four waves' in ascending
// order -- an order that (nA + nB) alone fixes, and no atomics.
__global__ __launch_bounds__(256) void score_pair_kernel(ScoreArgs a) {
    __shared__ float part[4];
    const int n = a.nA + a.nB;
    const float *cells = a.cells + blockIdx.z * (size_t)n;
    float sum = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) sum += cells[i];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) a.pair[blockIdx.z] = (((part[0] + part[1]) + part[2]) + part[3]) / (float)n;
}

void launch_score(const ScoreArgs &a, int batch, int normalize, hipStream_t stream) {
    const int col_groups = ceil_div(a.nB, MC_COLS);
    const dim3 grid(col_groups + ceil_div(a.nA, 4), 1, batch);
    if (normalize == P2P_SCORE_NONE) hipLaunchKernelGGL(score_cells_kernel<P2P_SCORE_NONE>, grid, dim3(256), 0, stream, a, col_groups);
    else if (normalize == P2P_SCORE_SOFTMAX) hipLaunchKernelGGL(score_cells_kernel<P2P_SCORE_SOFTMAX>, grid, dim3(256), 0, stream, a, col_groups);
    else hipLaunchKernelGGL(score_cells_kernel<P2P_SCORE_L1>, grid, dim3(256), 0, stream, a, col_groups);
    hipLaunchKernelGGL(score_pair_kernel, dim3(1, 1, batch), dim3(256), 0, stream, a);
}

}  // namespace p2p
