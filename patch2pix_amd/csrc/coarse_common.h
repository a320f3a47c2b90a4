// Shared by the coarse-stage sources: the kernels with their launchers (coarse.hip with matches.hip and score.hip, which it includes; consensus.hip;
// consensus_generic.hip, included by coarse.hip) and the host API over them (coarse_api.hip).  Every source that defines one of
// these functions includes this header, so a prototype that drifts from its definition does not compile.
#pragma once
#include "host_pack.h"
#include <algorithm>

namespace p2p {

struct NcGen;

// ---- coarse.hip: feature preparation, correlation + pooling, mutual matching (nz: pairs of the launch) -----------------------
struct PrepArgs {
    const float *F[2];
    unsigned short *Fn[2];
    int h[2], w[2];
    size_t sF[2];
    int C, k;
    size_t sFn;
    int *keys;
    int nkeys;
    size_t sKeys;
};
void launch_prep(const PrepArgs &a, unsigned nz, hipStream_t stream);
// delta: the argmax codes (ksize > 1; optional); sAB / sP / sDelta: per-pair strides of the feature planes, of P and of delta
int launch_corr_pool(const unsigned short *fnA, const unsigned short *fnB, int nA, int nB, int C, int ksize, float *P, uint8_t *delta,
                     size_t sAB, size_t sP, size_t sDelta, unsigned nz, hipStream_t stream);
void launch_maxima(const float *X, int nA, int nB, int *rkey, int *ckey, size_t sX, size_t sKeys, const float *X2, unsigned nz, hipStream_t stream);
void launch_mm_apply(const float *X, int nA, int nB, const int *rkey, const int *ckey, float *out, size_t sX, size_t sKeys,
                     size_t sOut, int *amax, const float *X2, size_t nz, hipStream_t stream);

// ---- matches.hip ------------------------------------------------------------------------------------------------------------
struct MatchArgs {
    const float *X;
    const uint8_t *delta;
    int hA, wA, hB, wB, ksize, upsample, center;
    long long *matches;
    float *scores;
    size_t sX, sM;      // per-pair strides: cells of the volume, rows of the match list
};
void launch_matches(const MatchArgs &m, int batch, hipStream_t stream);                                  // one candidate, softmax score
void launch_matches_topk(const MatchArgs &m, int batch, int topk, int do_softmax, hipStream_t stream);
void launch_delta_unpack(const uint8_t *delta, size_t n, int k, long long *out, hipStream_t stream);

// ---- score.hip --------------------------------------------------------------------------------------------------------------
struct ScoreArgs {
    const float *X;
    float *cells;       // [pairs][nA + nB], the A cells first
    float *pair;        // [pairs]
    int nA, nB;
    size_t sX;          // per-pair stride of the volume (cells)
};
void launch_score(const ScoreArgs &a, int batch, int normalize, hipStream_t stream);      // normalize: P2P_SCORE_*

// ---- consensus.hip: the fused kernel of the released stack --------------------------------------------------------------
void pack_nc_fused(const float *w1, const float *b1, const float *w2, DeviceBlob &out);      // lays out and fills the staging copy
int launch_nc_fused(const float *X, float *Y, float *Y2, size_t stride, int pairs, int d0, int d1, int d2, int d3,
                    const unsigned char *w_dev, float b2, const int *xmax, size_t xmax_stride, const int *forced_tile,
                    hipStream_t stream);
int launch_absmax(const float *x, size_t n, size_t stride, int pairs, int *out, size_t out_stride, hipStream_t stream);

// ---- consensus_generic.hip: any other stack, one launch per layer and branch (NcGen: the handle's layers, defined there) ----
int nc_generic_create(const p2p_ncn_config *cfg, const p2p_ncn_tensors *t, NcGen **out);
void nc_generic_destroy(NcGen *g);
size_t nc_generic_ws_bytes(const NcGen &g, size_t cells);
int launch_nc_generic(const NcGen &g, const float *X, size_t s_x, float *Y, size_t s_y, float *act, size_t s_act, int pairs,
                      int d0, int d1, int d2, int d3, hipStream_t stream);

}  // namespace p2p

// The opaque handle of include/p2p_hip.h: the fused kernel's weights or a generic stack.  `delete` frees either.
struct p2p_ncn {
    float b2;                // scalar bias of layer 2 (same for both branches)
    p2p::DeviceBlob wfused;  // both layers, both branches as fp16x2 MFMA fragments (consensus.hip)
    int tile[3];             // forced (ta, tb, tc) of the fused kernel, 0 = automatic (p2p_ncn_set_tile: tests and sweeps)
    p2p::NcGen *gen;         // a generic handle (p2p_ncn_create_config): its layers; the fields above are unused then
    ~p2p_ncn() { p2p::nc_generic_destroy(gen); }
};
