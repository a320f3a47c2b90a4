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
// planes: fp16 planes per operand, 2 (P2P_COARSE_FP16X2) or 1 (P2P_COARSE_FP16) -- the same for the three matrix-core launchers
// C: a multiple of 32 up to 1024 (above 256 the tile is dynamic LDS sized by C)
int launch_prep(const PrepArgs &a, int planes, unsigned nz, hipStream_t stream);
// delta: the argmax codes (ksize > 1; optional); sAB / sP / sDelta: per-pair strides of the feature planes, of P and of delta
int launch_corr_pool(const unsigned short *fnA, const unsigned short *fnB, int nA, int nB, int C, int ksize, int planes, float *P,
                     uint8_t *delta, size_t sAB, size_t sP, size_t sDelta, unsigned nz, hipStream_t stream);
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
                    const unsigned char *w_dev, float b2, const int *xmax, size_t xmax_stride, const int *forced_tile, int planes,
                    hipStream_t stream);
int launch_absmax(const float *x, size_t n, size_t stride, int pairs, int *out, size_t out_stride, hipStream_t stream);

// ---- consensus_generic.hip: any other stack, one launch per layer and branch (NcGen: the handle's layers, defined there) ----
int nc_generic_create(const p2p_ncn_config *cfg, const p2p_ncn_tensors *t, NcGen **out);
void nc_generic_destroy(NcGen *g);
// mode: the handle's (0 or P2P_COARSE_GENERIC_FP16X2, consensus_generic_h2.hip; its planes: nc_generic_ensure_h2, once)
size_t nc_generic_ws_bytes(const NcGen &g, size_t cells, int mode);
int nc_generic_ensure_h2(NcGen *g);
int launch_nc_generic(const NcGen &g, int mode, const float *X, size_t s_x, float *Y, size_t s_y, float *act, size_t s_act, int pairs,
                      int d0, int d1, int d2, int d3, hipStream_t stream);

// one stand-alone Conv4d layer (p2p_conv4d_*): the PLANAR form of the generic kernel (Conv4dLayer: defined there)
struct Conv4dLayer;
int conv4d_create(const float *weight, const float *bias, int c_in, int c_out, int k, Conv4dLayer **out);
void conv4d_destroy(Conv4dLayer *h);
void conv4d_dims(const Conv4dLayer &h, int *c_in, int *c_out);
int launch_conv4d(const Conv4dLayer &h, const float *x, float *y, int pairs, int d0, int d1, int d2, int d3, hipStream_t stream);

// ---- operators.hip: the matching operators as entry points of their own -----------------------------------------------------
struct CorrelationArgs {
    const float *A, *B;      // [item][C][nA], [item][C][nB]
    float *out;              // [item][nA][nB]
    int C, nA, nB;
    size_t sA, sB, sOut;     // floats between items
};
void launch_correlation(const CorrelationArgs &a, int batch, hipStream_t stream);
struct MaxPool4dArgs {
    const float *x;          // [item][p0 k][p1 k][p2 k][p3 k]
    float *pooled;           // [item][p0][p1][p2][p3]
    uint8_t *code;           // the same shape; optional
    int k, p1, p2, p3;
    size_t cells;            // pooled cells per item
};
void launch_maxpool4d(const MaxPool4dArgs &a, int batch, hipStream_t stream);
void launch_l2_normalize(const float *x, size_t outer, int C, size_t inner, float *y, hipStream_t stream);
// keys: per item sKeys = roundup4(nA) + roundup4(nB) words (row keys, then column keys)
void launch_mutual_matching(const float *x, int nA, int nB, float *y, int *keys, size_t sKeys, int batch, hipStream_t stream);

}  // namespace p2p

// The opaque handle of include/p2p_hip.h: the fused kernel's weights or a generic stack.  `delete` frees either.
struct p2p_ncn {
    float b2;                // scalar bias of layer 2 (same for both branches)
    p2p::DeviceBlob wfused;  // both layers, both branches as fp16x2 MFMA fragments (consensus.hip)
    int tile[3];             // forced (ta, tb, tc) of the fused kernel, 0 = automatic (p2p_ncn_set_tile: tests and sweeps)
    p2p::NcGen *gen;         // a generic handle (p2p_ncn_create_config): its layers; the fields above are unused then
    int mode = 0;            // P2P_COARSE_FP16X2 / P2P_COARSE_FP16 (p2p_ncn_set_mode): planes per operand of the matrix-core kernels;
                             // a generic handle: 0 (exact fp32) or P2P_COARSE_GENERIC_FP16X2
    ~p2p_ncn() { p2p::nc_generic_destroy(gen); }
};

// One Conv4d layer (p2p_conv4d_create)
struct p2p_conv4d {
    p2p::Conv4dLayer *layer;
    ~p2p_conv4d() { p2p::conv4d_destroy(layer); }
};
