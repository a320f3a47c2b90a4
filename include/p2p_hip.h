/*
 * libp2p_hip -- MI355X (gfx950) implementation of the Patch2Pix matching hot path.
 *
 * C ABI, plain pointers and sizes only.  The reference (GrumpyZhou/patch2pix) has no FFI: its
 * boundary for this path is the Python module API (networks/patch2pix.py, utils/eval/model_helper.py).
 * Each entry point below names the reference function(s) it replaces; the Python side
 * (patch2pix_amd/) binds them with ctypes and re-exposes the reference's own names.
 *
 * Conventions
 *   - every function returns 0 on success or a negative P2P_E* code; p2p_last_error() returns a
 *     thread-local message for the last failure on the calling thread;
 *   - "device pointer" arguments are caller-owned HBM buffers (torch tensors); nothing is retained
 *     across calls except the opaque weight handles;
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - threading: every launch function is re-entrant per stream and may be called from several host threads (distinct
 *     streams, or one stream with the caller's own ordering); the weight handles are immutable after creation
 *     (p2p_regressor_set_mode / p2p_ncn_set_tile / p2p_ncn_set_mode / p2p_conv_set_tile / p2p_conv_set_mode / p2p_stem_set_mode mutate a
 *     handle and must not race with launches that use it).  The only process-wide state is a per-device "kernel attributes set" flag per launcher (dynamic-LDS size via
 *     hipFuncSetAttribute, compute-unit count): atomic, set after idempotent work, so two threads meeting on a device's
 *     first launch both do that work and neither sees a half-initialised value;
 *   - dense tensors are contiguous fp32 in the layout PyTorch produces (NCHW without the N);
 *   - match rows are (xA, yA, xB, yB).
 */
#ifndef P2P_HIP_H
#define P2P_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2P_OK            0
#define P2P_EINVAL       -1   /* bad argument (null pointer, size not supported ...) */
#define P2P_EHIP         -2   /* a HIP runtime call failed */
#define P2P_EUNSUPPORTED -3   /* valid for the reference but not implemented by this library */
#define P2P_ENOMEM       -4   /* workspace too small / allocation failed */

typedef void *p2p_stream_t;                 /* hipStream_t */
typedef struct p2p_ncn p2p_ncn;             /* NCNet consensus filters, device resident */
typedef struct p2p_regressor p2p_regressor; /* one FeatRegressNet, packed + device resident */

int p2p_version(void);
const char *p2p_last_error(void);

/* ---- weights ------------------------------------------------------------------------------- */

/* NeighConsensus(kernel_sizes=[3,3], channels=[16,1]) -- reference networks/ncn/model.py:124-143,
 * built at networks/patch2pix.py:32.  HOST pointers to the checkpoint tensors in their stored
 * (pre-permuted, networks/ncn/conv4d.py:119-120) layout:
 *   w1 [3,16,1,3,3,3]  b1 [16]  w2 [3,1,16,3,3,3]  b2 [1]                                     */
int p2p_ncn_create(const float *w1, const float *b1, const float *w2, const float *b2, p2p_ncn **out);
void p2p_ncn_destroy(p2p_ncn *ncn);
/* Tests and sweeps: force the work-group tile (ta, tb, tc) of the consensus kernel for launches with this handle (0, 0, 0 =
 * automatic; ta = 0 with tb, tc > 0: only the march length is picked; any other partial triple is P2P_EINVAL).  Results do not depend on the tile: every output
 * cell sums its contributions in one fixed order.                                                                   */
int p2p_ncn_set_tile(p2p_ncn *ncn, int ta, int tb, int tc);

/* Any other NeighConsensus(kernel_sizes, channels, symmetric_mode) within these limits (since version 106) -- a GENERIC handle
 * (csrc/consensus_generic.hip: exact fp32 on v_mfma_f32_16x16x4_f32, one launch per layer and branch, the hidden activations
 * in the caller's workspace):
 *   n_layers     1..4
 *   kernel_size  3 or 5 per layer (cubic in all four axes, as the reference builds them)
 *   channels     output channels per layer: 1..16 for the hidden layers, 1 for the last one (the volume is [B,1,...] downstream)
 *   symmetric    non-zero: y = net(x) + T(net(T(x))) (model.py:149); zero: y = net(x)
 * HOST pointers to the checkpoint tensors in their stored layout: w[i] [k, c_out, c_in, k, k, k] (conv4d.py:119-120), b[i] [c_out].
 * Kernel sizes, channel counts or layer counts outside these lists -> P2P_EUNSUPPORTED; null pointers and counts or dims <= 0 ->
 * P2P_EINVAL; both before the device is touched.  The released shape is accepted too (that is how the generic path is compared
 * with the tuned one); p2p_ncn_create keeps producing tuned handles.  Every coarse entry point takes either kind;
 * p2p_ncn_set_tile refuses a generic handle (P2P_EUNSUPPORTED).  A generic handle's results do not depend on the batch, the
 * pair's position in it or the workspace size: every output cell sums its terms in an order the configuration alone fixes.
 * Like every constructor of this library it packs on the host and uploads once: a device allocation that fails -> P2P_ENOMEM,
 * a copy that fails -> P2P_EHIP (nothing stays allocated). */
typedef struct p2p_ncn_config { int n_layers, kernel_size[4], channels[4], symmetric; } p2p_ncn_config;
typedef struct p2p_ncn_tensors { const float *w[4], *b[4]; } p2p_ncn_tensors;
int p2p_ncn_create_config(const p2p_ncn_config *config, const p2p_ncn_tensors *tensors, p2p_ncn **out);
int p2p_ncn_is_generic(const p2p_ncn *ncn);      /* 1 / 0; -1 for NULL */

/* The arithmetic of the matrix-core kernels of a coarse-stage call made with this handle (p2p_coarse_forward,
 * p2p_coarse_forward_batch, p2p_neigh_consensus_batch).  P2P_COARSE_FP16X2 is the default: fp32-equivalent, two fp16 planes
 * per operand and three MFMA products per fp32 product.  P2P_COARSE_FP16 is opt-in and NOT fp32-equivalent: the same kernels
 * with ONE fp16 plane per operand (the normalised features, the consensus input, its weights and its hidden volume each
 * rounded once to fp16 behind the same exact power-of-two scales: 2^-11 relative) and one MFMA product; accumulation and
 * every epilogue stay fp32.  Winners of near-ties may move; the index / 1e-3 px bars of the default mode do not apply.
 * Tile, strip walk and summation order are the default mode's: a result does not depend on the tile, the batch or the
 * workspace size in either mode.  Nothing is re-packed or uploaded on a change (the packed weights hold plane 0 already).
 * Mutual matching, match extraction, the scores and the operator entry points (p2p_correlation_batch, p2p_conv4d_*,
 * p2p_maxpool4d_batch) are not affected.  An unknown mode -> P2P_EINVAL; P2P_COARSE_FP16 on a generic handle ->
 * P2P_EUNSUPPORTED; NULL -> P2P_EINVAL from the setter, -1 from the getter.
 * A generic handle (p2p_ncn_create_config) has two modes of its own.  0 is its default arithmetic: exact fp32 MFMA.
 * P2P_COARSE_GENERIC_FP16X2 is opt-in and fp32-equivalent: every layer behind the first (more than one input channel) runs on
 * the fp16 matrix cores with two fp16 planes per operand and three MFMA products -- the weights under one exact power of two
 * per output channel, a layer's input under one power of two per PAIR (the largest magnitude the producing layer stored for
 * that pair), fp32 accumulation in an order the configuration alone fixes; the first layer stays exact, so a single-layer
 * stack computes the same bits in both modes.  A pair's result does not depend on the batch, its position or the workspace
 * size; a non-finite value stays inside its own pair.  The planes are packed and uploaded on the first selection (a failure
 * there -> P2P_ENOMEM / P2P_EHIP, the mode unchanged).  The mode needs a little more workspace: query
 * p2p_coarse_workspace_bytes_for / p2p_neigh_consensus_workspace_bytes again after a mode change.  On a tuned handle the id
 * is P2P_EUNSUPPORTED.  p2p_conv4d_* is not affected.                                                                      */
#define P2P_COARSE_FP16X2 0
#define P2P_COARSE_FP16   1
#define P2P_COARSE_GENERIC_FP16X2 17
int p2p_ncn_set_mode(p2p_ncn *ncn, int mode);
int p2p_ncn_get_mode(const p2p_ncn *ncn);

/* FeatRegressNet with the released configuration (conv_kers [3,3], conv_strs [2,1],
 * conv_dims [512,512], fc_dims [512,256], feat_comb 'pre', psize 16, feat_idx [0,1,2,3]) --
 * reference networks/modules.py:56-112.  HOST pointers to the state_dict tensors.  These handles run the tuned kernels
 * (the modes below); every other configuration goes through p2p_regressor_create_config.     */
typedef struct p2p_bn_params {
    const float *weight, *bias, *running_mean, *running_var;
} p2p_bn_params;

typedef struct p2p_regressor_params {
    const float *conv1_w;      /* conv.0.weight [512,518,3,3] */
    p2p_bn_params bn1;         /* conv.1.*      [512]         */
    const float *conv2_w;      /* conv.2.weight [512,512,3,3] */
    p2p_bn_params bn2;         /* conv.3.*      [512]         */
    const float *fc1_w, *fc1_b; /* fc.0 [512,512],[512]       */
    p2p_bn_params bnf1;        /* fc.1.*        [512]         */
    const float *fc2_w, *fc2_b; /* fc.3 [256,512],[256]       */
    p2p_bn_params bnf2;        /* fc.4.*        [256]         */
    const float *fc3_w, *fc3_b; /* fc.6 [5,256],[5]           */
} p2p_regressor_params;

int p2p_regressor_create(const p2p_regressor_params *params, p2p_regressor **out);
void p2p_regressor_destroy(p2p_regressor *reg);

/* Arithmetic used for the two convolutions of a regressor (everything else is fp32 either way; the
 * reference computes them in fp32, networks/modules.py:76-87):
 *   P2P_REGRESS_FP16X2 fp32-equivalent on the fp16 matrix cores: every fp32 operand, scaled by an exact power of
 *                      two into the normal range of fp16, is the sum of two fp16 numbers to within 2^-24 of its
 *                      magnitude; three v_mfma_f32_32x32x16_f16 per product (the dropped term is <= 2^-24 of it),
 *                      fp32 accumulation; the scales are undone exactly.  As accurate as P2P_REGRESS_F32 against
 *                      an fp64 evaluation at 5.3x its matrix-core ceiling;
 *   P2P_REGRESS_F32    v_mfma_f32_32x32x2_f32, bit-identical to an fp32 fma chain;
 *   P2P_REGRESS_FP16X2W (default) the same arithmetic with the second convolution (3x3, stride 1 on the 8x8 map) evaluated as
 *                      Winograd F(2x2, 3x3): 16 batched GEMMs over the transformed tiles of ALL proposals (2.25x fewer
 *                      matrix-core passes; the transforms are exact up to fp32 rounding, transformed filters computed in
 *                      fp64 at pack time) -- three launches per regressor level instead of one, and a larger scratch
 *                      buffer (the transformed conv2 input of a chunk of up to 3328 proposals, 512 KiB each);
 *   P2P_REGRESS_FP16   (opt-in, since version 111; NOT fp32-equivalent) the structure of P2P_REGRESS_FP16X2W with ONE fp16
 *                      number per operand -- fp16(x * 2^s) under the same power-of-two scales -- and ONE
 *                      v_mfma_f32_32x32x16_f16 per product, fp32 accumulation: a third of the matrix-core passes, half the
 *                      operand bytes, relative operand rounding 2^-11.  Its results are NOT held to the 1e-3 px / 1e-5 bars
 *                      of the other modes (measured error: DESIGN.md section 4, "Single-plane mode").  Tuned handles only.
 * New handles start in P2P_REGRESS_DEFAULT (the library reads no environment variables; the Python host layer maps
 * P2P_REGRESS_MODE onto p2p_regressor_set_mode).  Only the weight stream of the mode in use is packed and uploaded;
 * p2p_regressor_set_mode builds another mode's on its first selection (host-side packing + one upload).   */
#define P2P_REGRESS_F32     0
#define P2P_REGRESS_FP16X2  3
#define P2P_REGRESS_FP16X2W 4
#define P2P_REGRESS_FP16    5
#define P2P_REGRESS_DEFAULT P2P_REGRESS_FP16X2W
int p2p_regressor_set_mode(p2p_regressor *reg, int mode);
int p2p_regressor_get_mode(const p2p_regressor *reg);

/* FeatRegressNet with ANY configuration within the limits below (since version 104): what the reference's training script
 * stores as `feat_idx` / `regressor_config` of a checkpoint (utils/eval/model_helper.py:28-62).  Such a GENERIC handle runs
 * a second, shape-generic set of kernels behind the same p2p_regress* entry points: exact fp32 on the matrix cores
 * (v_mfma_f32_32x32x2_f32 for the convolutions as implicit GEMMs, v_mfma_f32_16x16x4_f32 for the FC tail), one launch per
 * layer over a chunk of proposals.  Every output's summation order depends on the configuration alone: a proposal's raw
 * outputs are bit-identical alone, in any batch, with device-side counts and under any chunk size.
 *   feat_idx   n_feat in [1,4] strictly ascending levels out of {0,1,2,3} (3 / 64 / 64 / 128 channels, strides 1 / 2 / 4 / 8);
 *              the per-pixel L2 norm runs over the selected channels.  Level 4 -> P2P_EUNSUPPORTED (p2p_pyramid has 4 levels)
 *   feat_comb  P2P_FEAT_COMB_PRE: one conv stack on cat(f1, f2); P2P_FEAT_COMB_POST: the stack on each image's patch, the
 *              two pooled vectors concatenated (fc input = 2 conv_dim[n_conv - 1])
 *   conv       n_conv in [1,4] layers Conv2d(kernel conv_ker in {1,3,5}, stride conv_str in {1,2}, padding 1, no bias) +
 *              BatchNorm2d; ONE ReLU after the last BatchNorm, then the maximum over the final map.  conv_dim: multiples of
 *              16 in [16,1024].  A map that would shrink below 1x1 -> P2P_EINVAL
 *   fc         n_fc in [0,4] hidden layers Linear + BatchNorm1d + ReLU, fc_dim multiples of 16 in [16,1024]; then Linear to 5
 *   psize      16 (anything else -> P2P_EUNSUPPORTED)
 * Kernel sizes, strides, dims or layer counts outside these lists -> P2P_EUNSUPPORTED; malformed arguments (null pointers,
 * counts or dims <= 0, feat_idx out of order) -> P2P_EINVAL.  The released configuration is accepted too (that is how the
 * generic path is compared with the tuned one); p2p_regressor_create keeps producing tuned handles.
 * Tensors: HOST pointers to the state_dict tensors, conv_w[i] = conv.{2i}.weight [conv_dim[i], c_in, k, k] (c_in of layer 0:
 * the selected channels, twice for 'pre'), conv_bn[i] = conv.{2i+1}.*, fc_w/fc_b[i] = fc.{3i}.*, fc_bn[i] = fc.{3i+1}.*,
 * out_w/out_b = fc.{3 n_fc}.* [5, k], [5].  A device allocation that fails -> P2P_ENOMEM, a copy that fails -> P2P_EHIP
 * (every constructor of the library; p2p_regressor_set_mode, which uploads a mode's weight stream on its first selection, too). */
#define P2P_FEAT_COMB_PRE  0
#define P2P_FEAT_COMB_POST 1
typedef struct p2p_regressor_config {
    int n_feat, feat_idx[4];
    int feat_comb;
    int n_conv, conv_dim[4], conv_ker[4], conv_str[4];
    int n_fc, fc_dim[4];
    int psize;
} p2p_regressor_config;
typedef struct p2p_regressor_tensors {
    const float *conv_w[4];
    p2p_bn_params conv_bn[4];
    const float *fc_w[4], *fc_b[4];
    p2p_bn_params fc_bn[4];
    const float *out_w, *out_b;
} p2p_regressor_tensors;
int p2p_regressor_create_config(const p2p_regressor_config *config, const p2p_regressor_tensors *tensors, p2p_regressor **out);
/* The mode ids of a generic handle.  New generic handles start in P2P_REGRESS_GENERIC (exact fp32, above).
 *   P2P_REGRESS_GENERIC_FP16X2 (opt-in, fp32-equivalent) runs the convolution stack on v_mfma_f32_32x32x16_f16 with the scheme of
 *     P2P_REGRESS_FP16X2: every fp32 operand, scaled by an exact power of two, as two fp16 planes, three MFMA products per
 *     fp32 product (a0 b0 + a0 b1 + a1 b0), fp32 accumulation.  Weights carry a per-output-channel exponent folded into the
 *     BatchNorm scale; layer 0 reads the L2-normalised patches under the fixed scale 2^12; an inner layer reads its input
 *     under a per-SAMPLE power of two derived from the largest magnitude the producing layer stored for that sample.  The
 *     gather, the FC tail and the final Linear are those of P2P_REGRESS_GENERIC.  Outputs stay a function of the proposal and
 *     the configuration alone (bit-identical alone, in any batch, with device-side counts, under any chunk size), but they
 *     are NOT the bits of P2P_REGRESS_GENERIC; both modes are held to the same bars.
 * p2p_regressor_set_mode on a generic handle accepts these two ids (the first selection of P2P_REGRESS_GENERIC_FP16X2 packs
 * and uploads its weight planes; going back to P2P_REGRESS_GENERIC gives the handle's earlier outputs bit for bit), answers
 * P2P_EUNSUPPORTED for the ids of the tuned modes and P2P_EINVAL for an id the library does not know.  A tuned handle
 * refuses both generic ids (P2P_EUNSUPPORTED).  p2p_regressor_get_mode returns the current id.  In p2p_regress* reg1 and
 * reg2 must be of the same kind, two generic handles must have equal configurations and be in the same mode (P2P_EINVAL
 * otherwise; the message names both modes).                                                                          */
#define P2P_REGRESS_GENERIC 16
#define P2P_REGRESS_GENERIC_FP16X2 17

/* ---- coarse stage ---------------------------------------------------------------------------- */

/* Workspace (bytes) p2p_coarse_forward needs for these sizes (per pair); ksize 1, 2 or 4. */
size_t p2p_coarse_workspace_bytes(int channels, int hA, int wA, int hB, int wB, int ksize);
/* The same for a given handle: a generic handle adds the two activation buffers of its widest hidden layer (fp32, channels
 * padded to 4, 8 or 16, per pooled cell); for a tuned handle the value above.  0 for bad arguments. */
size_t p2p_coarse_workspace_bytes_for(const p2p_ncn *ncn, int channels, int hA, int wA, int hB, int wB, int ksize);
/* Workspace (bytes) p2p_neigh_consensus_batch needs PER VOLUME of these sizes: 4 for a tuned handle, the activation buffers
 * for a generic one.  0 for bad arguments. */
size_t p2p_neigh_consensus_workspace_bytes(const p2p_ncn *ncn, int hA, int wA, int hB, int wB);

/* Patch2Pix.forward_coarse_match -- reference networks/patch2pix.py:120-136:
 * L2Normalize (modules.py:6) -> FeatCorrelation (modules.py:41-53) -> maxpool4d (modules.py:11-34,
 * only if ksize > 1) -> MutualMatching (ncn/model.py:157-176) -> NeighConsensus (ncn/model.py:145-155,
 * conv4d.py:12-74) -> MutualMatching.
 *   featA [C,hA,wA], featB [C,hB,wB]      device, fp32
 *   corr4d_out [hA/k, wA/k, hB/k, wB/k]   device, fp32
 *   delta_out  same shape, uint8, value s = ((di*k+dj)*k+dk)*k+dl of the first maximum in the
 *              reference's slice order (modules.py:13-18); may be NULL; ignored when ksize == 1
 * ksize must be 1, 2 (the reference's default in predict_*) or 4 (maxpool4d's own default; since version 103);
 * other values -> P2P_EUNSUPPORTED (k^4 codes must fit the byte: 4 is the last value that does).  Feature map sides
 * must be multiples of ksize (P2P_EINVAL otherwise).
 * channels: a multiple of 32 up to 1024 (P2P_EUNSUPPORTED otherwise) -- 256 for ResNet34, 1024 for ResNet50 / ResNet101
 * truncated after layer3 (NCNet's own configuration); in both coarse modes.  Above 256 channels the feature-preparation
 * kernel keeps a position's channels in dynamic LDS sized by the channel count; the sum of squares is one fixed-order fp32
 * reduction per position at every width, so a pair's result does not depend on its batch mates or on the tiling.  Up to
 * 256 channels the buffers and results are bit for bit those of the versions that stopped there.             */
int p2p_coarse_forward(const float *featA, const float *featB, int channels, int hA, int wA, int hB, int wB,
                       int ksize, const p2p_ncn *ncn, float *corr4d_out, uint8_t *delta_out,
                       void *workspace, size_t workspace_bytes, p2p_stream_t stream);

/* The same for the batch axis of the reference's tensors (feat1/feat2 are [B,C,h,w] in
 * networks/patch2pix.py:120-136): `batch` equally sized pairs, contiguous along the leading axis in all four
 * arrays, one launch per kernel for the whole batch.  The workspace must hold at least one pair
 * (p2p_coarse_workspace_bytes); with batch x that size all pairs are processed together, with less they are
 * processed in as many groups as fit.  ksize: 1, 2 or 4, as above.                                */
int p2p_coarse_forward_batch(const float *featA, const float *featB, int batch, int channels, int hA, int wA, int hB,
                             int wB, int ksize, const p2p_ncn *ncn, float *corr4d_out, uint8_t *delta_out,
                             void *workspace, size_t workspace_bytes, p2p_stream_t stream);

/* NeighConsensus.forward -- reference networks/ncn/model.py:145-155 (kernel_sizes [3,3], channels [16,1]):
 * y = net(x) + T(net(T(x))), net = Conv4d(1->16) + ReLU + Conv4d(16->1) + ReLU (conv4d.py:12-74), T = swap of the A and B axes,
 * on `batch` volumes x [B, hA, wA, hB, wB] (fp32) -> y_out of the same shape.  One kernel on the fp16 matrix cores in
 * fp32-equivalent arithmetic (the fp16 planes are scaled by the volume's largest magnitude, found first); the hidden
 * 16-channel volume stays in LDS (csrc/consensus.hip).  workspace: 4 bytes per volume of device memory.
 * With a generic handle: the handle's own stack, layer by layer in exact fp32; the workspace must hold at least one volume's
 * p2p_neigh_consensus_workspace_bytes (P2P_ENOMEM below that); with less than batch x that, the volumes go in groups.
 * The workspace of a generic handle must be 16-byte aligned, here and in p2p_coarse_forward* (P2P_EINVAL otherwise: the
 * activations are read with 16-byte loads; any hipMalloc pointer is). */
int p2p_neigh_consensus_batch(const float *x, int batch, int hA, int wA, int hB, int wB, const p2p_ncn *ncn, float *y_out,
                              void *workspace, size_t workspace_bytes, p2p_stream_t stream);

/* Expand the packed relocalisation byte into the reference's four int64 tensors
 * (max_i, max_j, max_k, max_l of modules.py:24-28); `out` holds 4 consecutive planes of n int64.
 * ksize: the one the byte was packed with (1, 2 or 4 from p2p_coarse_forward; code 255 = (3,3,3,3) at ksize 4). */
int p2p_delta_unpack(const uint8_t *delta, size_t n, int ksize, int64_t *out, p2p_stream_t stream);

/* Patch2Pix.cal_coarse_matches -- reference networks/patch2pix.py:340-375, i.e. corr_to_matches in
 * both directions (ncn/extract_ncmatches.py:6-94: softmax along one side, max/first-argmax,
 * relocalisation with delta) concatenated B->A first then A->B, scaled to pixels:
 *   matches_out [nB + nA, 4] int64 = upsample * (xA,yA,xB,yB) (+ upsample/2 if center)
 *   scores_out  [nB + nA]    fp32                                    (nA = hA'*wA', nB = hB'*wB')
 * corr4d dims are the pooled ones; delta may be NULL (ksize 1); ksize 1, 2 or 4 (batch form alike). */
int p2p_coarse_matches(const float *corr4d, const uint8_t *delta, int hA, int wA, int hB, int wB, int ksize,
                       int upsample, int center, int64_t *matches_out, float *scores_out, p2p_stream_t stream);

/* Batch form: corr4d [B, ...], delta [B, ...], matches_out [B, nB + nA, 4], scores_out [B, nB + nA]. */
int p2p_coarse_matches_batch(const float *corr4d, const uint8_t *delta, int batch, int hA, int wA, int hB, int wB,
                             int ksize, int upsample, int center, int64_t *matches_out, float *scores_out,
                             p2p_stream_t stream);

/* The topk best candidates per cell and direction, and raw scores (since version 105) -- reference
 * ncn/extract_ncmatches.py:96-158 (corr_to_matches_topk) in both directions, concatenated B->A first then A->B the way
 * cal_coarse_matches concatenates corr_to_matches; do_softmax = 0 is the `do_softmax=False` of both extractors (:30, :45,
 * :111, :126): the score is the consensus value itself, bit for bit.  With nA = hA'*wA', nB = hB'*wB' per pair:
 *   matches_out [B, topk*(nB+nA), 4] int64, scores_out [B, topk*(nB+nA)] fp32
 *   row t*nB + c             rank t of B cell c among the A cells     (the reference's view(batch, topk, -1))
 *   row topk*nB + r*topk + t rank t of A cell r among the B cells     (view(batch, -1, topk))
 * Order within a column / row: descending value; equal values by ascending flat cell index.  torch.topk leaves ties
 * unspecified, so this is the library's definition; it extends the "first index attaining the maximum" of the two
 * functions above.  Only values above -inf are candidates (NaN compares false and is none either): a column / row with
 * fewer than topk of them repeats, from the first missing rank on, one clamped cell (the last of the other image) with
 * score -inf (do_softmax = 0) or 0 (do_softmax = 1; NaN if no value is above -inf).  Softmax scores are expf(x_t - max) / sum expf(x - max) with the sum taken exactly as those functions
 * take it: topk = 1 with do_softmax = 1 gives their matches and scores bit for bit.
 * 1 <= topk <= 8 and topk <= min(nA, nB) (torch.topk raises beyond that as well), else P2P_EINVAL; every other argument as
 * in the batch form above.  One pass over the volume per rank (csrc/matches.hip).                        */
int p2p_coarse_matches_topk_batch(const float *corr4d, const uint8_t *delta, int batch, int hA, int wA, int hB, int wB,
                                  int ksize, int upsample, int center, int topk, int do_softmax,
                                  int64_t *matches_out, float *scores_out, p2p_stream_t stream);

/* Patch2Pix.cal_coarse_score -- reference networks/patch2pix.py:320-338 (since version 108): the NCNet pair score, the mean
 * over all cells of both images of the best normalised consensus value, per pair.  With X[b] the volume of pair b as an
 * [nA][nB] matrix (nA = hA*wA, nB = hB*wB, the dims of corr4d as given) and N the normalisation taken along the axis the
 * maximum runs over:
 *   column scores  sB[b][c] = max_a N_a(X[b][a][c])      row scores  sA[b][r] = max_c N_c(X[b][r][c])
 *   cell_scores [B, nA + nB] fp32 = sA then sB per pair, the order of the reference's torch.cat([scores_A, scores_B]);
 *                              optional (NULL: the cell scores pass through `workspace`)
 *   pair_scores [B] fp32     = the mean of the pair's nA + nB cell scores; required.  The reference's scalar is the mean of
 *                              these B values (every pair of a batch has the same cell count).
 *   P2P_SCORE_NONE     N = identity: the maximum itself, bit for bit (`normalize=None`)
 *   P2P_SCORE_SOFTMAX  1 / sum expf(x - max), the sum taken over the same slices in the same order as p2p_coarse_matches_batch
 *                      takes it: a cell's score is the score that call returns for the cell, bit for bit
 *   P2P_SCORE_L1       max(x / (sum x + 0.0001)).  A correctly rounded division is monotone, so this is max(x) / d for
 *                      d = sum x + 0.0001 > 0 and min(x) / d for d < 0: maximum, minimum and sum come from one scan, then one
 *                      IEEE division.  The volume need not be non-negative; d == 0 gives what IEEE gives.
 * Summation and order: a pair's nA + nB cell scores are added in an order that (nA, nB) alone fixes -- thread t of one
 * 256-thread work-group per pair adds cells t, t + 256, ... ascending, a wave its 64 partial sums in an xor tree, then the four
 * waves ascending; no float atomics.  It depends neither on B, nor on the pair's slot in the batch, nor on the launch shape: a
 * pair's cell and pair scores are bit-identical alone and in any batch.
 * workspace: device memory, 4-byte aligned, p2p_coarse_score_workspace_bytes bytes (B x (nA + nB) floats), needed only when
 * cell_scores is NULL (P2P_ENOMEM if it is missing or too small); ignored otherwise (NULL, 0 allowed).  Null corr4d or
 * pair_scores, batch outside 1..65535, non-positive dims and an unknown normalisation -> P2P_EINVAL; all before the device is
 * touched.  Two launches (csrc/score.hip), asynchronous on `stream`.  The query returns 0 for bad arguments. */
#define P2P_SCORE_NONE    0
#define P2P_SCORE_SOFTMAX 1
#define P2P_SCORE_L1      2
size_t p2p_coarse_score_workspace_bytes(int batch, int hA, int wA, int hB, int wB);
int p2p_coarse_score_batch(const float *corr4d, int batch, int hA, int wA, int hB, int wB, int normalize,
                           float *cell_scores, float *pair_scores, void *workspace, size_t workspace_bytes,
                           p2p_stream_t stream);

/* filter_coarse -- reference networks/utils.py:38-72 without the `ptmax` sampling (which draws from the host's numpy
 * RNG and therefore stays on the host): per batch item the lexicographically sorted distinct rows of matches [n,4]
 * with the score of their first occurrence; `mutual` keeps rows that occur more than once; an empty selection leaves
 * the list as it was; then rows with score > ncn_thres, again "or everything".
 *   matches [B,n,4] int64, scores [B,n] fp32  ->  out_matches [B,n,4], out_scores [B,n] (first out_counts[b] rows
 *   valid), out_counts [B] int32 on the device; out_counts[b] = -1 if a coordinate is negative or >= 2^15 (the caller
 *   falls back to the host path).
 * Lists of up to 8192 rows are filtered entirely in LDS and need no workspace (NULL, 0).  Longer lists (a 960x1280 pair
 * at ksize 2 has 9600 rows) are sorted in `workspace`, p2p_filter_coarse_workspace_bytes(batch, n) bytes of device
 * memory (0 for n <= 8192; P2P_ENOMEM if it is missing or too small); n <= 2^20.                                  */
size_t p2p_filter_coarse_workspace_bytes(int batch, int n);
int p2p_filter_coarse_batch(const int64_t *matches, const float *scores, int batch, int n, float ncn_thres, int mutual,
                            int64_t *out_matches, float *out_scores, int *out_counts, void *workspace,
                            size_t workspace_bytes, p2p_stream_t stream);

/* The tail of estimate_matches -- reference utils/eval/model_helper.py:92-109 -- for a batch with device-side counts:
 * per item keep the rows with fine score > io_thres (all rows if none passes), in order, and scale refined and coarse
 * coordinates to original-image pixels in float64.
 *   fine [B,stride,4] fp32, scores [B,stride] fp32, coarse [B,stride,4] int64, counts [B] int32 (device; valid rows per
 *   item, -1 passes through), scale [B,4] float64 (device; w1o/w1, h1o/h1, w2o/w2, h2o/h2)
 *   -> out_matches [B,stride,4] f64, out_scores [B,stride] fp32, out_coarse [B,stride,4] f64, out_counts [B] int32.   */
int p2p_match_tail_batch(const float *fine, const float *scores, const int64_t *coarse, const int *counts,
                         const double *scale, int batch, int stride, float io_thres, double *out_matches,
                         float *out_scores, double *out_coarse, int *out_counts, p2p_stream_t stream);

/* Epipolar evaluation of match rows -- reference utils/eval/measure.py:18-71 (sampson_distance, symmetric_epipolar_distance),
 * networks/utils.py:74-110 (sym_epi_dist, sampson_dist) and the np.histogram of check_inliers_distr (measure.py:115-141)
 * (since version 109): per row (x1, y1, x2, y2) the distance to the epipolar geometry of the item's fundamental matrix, and per
 * item the bin counts of those distances.  The inputs have the layout p2p_match_tail_batch leaves on the device.
 *   matches [B,stride,4]  P2P_F64, P2P_F32 or P2P_I64 (matches_dtype), device
 *   counts  [B] int32     device; valid rows per item.  -1 passes through: the item's hist row is zeros, its dist row untouched;
 *                         0: the hist row is zeros.  A count above stride is read as stride
 *   F       [B,9] fp64    device, row-major, x2^T F x1 = 0
 *   edges   [nbins+1] fp64 device, ascending; together with hist, or both NULL (then nbins = 0)
 *   dist    [B,stride]    P2P_F64 or P2P_F32 (dist_dtype); the first counts[b] entries of an item are written, the others left
 *   hist    [B,nbins] int32, optional
 * With the homogeneous third coordinate 1, l2 = F x1, l1 = F^T x2 and dd = x2 . l2:
 *   P2P_EPI_SAMPSON   dd^2 / (eps + l1_0^2 + l1_1^2 + l2_0^2 + l2_1^2)              measure.py:39, networks/utils.py:109
 *   P2P_EPI_SYM       dd^2 (1 / (eps + l1_0^2 + l1_1^2) + 1 / (eps + l2_0^2 + l2_1^2))     measure.py:70, networks/utils.py:92
 *   P2P_EPI_SYM_SQRT  |dd| (1 / sqrt(eps + l1_0^2 + l1_1^2) + 1 / sqrt(eps + l2_0^2 + l2_1^2))   measure.py:67, networks/utils.py:90
 *   P2P_EPI_VALUE     x1 itself: the first column holds distances computed earlier, which are stored and binned (the bin counts
 *                     of check_inliers_distr for arrays that are distances already); F and eps are checked and not used
 * eps = 0 is the numpy symmetric_epipolar_distance (which has no eps), 1e-8 the default of the other three functions.  A zero
 * denominator gives what IEEE gives (0 / 0 = NaN, x / 0 = inf).
 * ONE arithmetic, whatever the types: every input is widened to fp64 (exact for fp32; int64 beyond 2^53 rounds to nearest),
 * everything is computed in fp64 in the order below -- fma is the fused operation, every other operation one IEEE operation,
 * nothing is left to the compiler's contraction -- and the result is rounded once if dist is fp32 (the reference's d.float()):
 *   l2_i = fma(F[3i], x1, fma(F[3i+1], y1, F[3i+2]))   i = 0, 1, 2        l1_j = fma(F[j], x2, fma(F[3+j], y2, F[6+j]))   j = 0, 1
 *   dd = fma(x2, l2_0, fma(y2, l2_1, l2_2))     s1 = fma(l1_1, l1_1, l1_0 * l1_0)     s2 = fma(l2_1, l2_1, l2_0 * l2_0)
 *   SAMPSON   (dd * dd) / ((eps + s1) + s2)
 *   SYM       (dd * dd) * (1 / (eps + s1) + 1 / (eps + s2))
 *   SYM_SQRT  fabs(dd) * (1 / sqrt(eps + s1) + 1 / sqrt(eps + s2))
 * Histogram: np.histogram(dist, edges)[0] of the values AS STORED (after the rounding to fp32 if dist is fp32): bin i is
 * [e_i, e_i+1), the last bin is closed on the right, values outside [e_0, e_nbins] and NaNs are not counted.  1 <= nbins <= 16.
 * Counts are added with integer atomics in LDS only: they do not depend on any order.  Edges that do not ascend are the caller's
 * error and cannot be seen on the host (the pointer is a device pointer): the counts are then meaningless, nothing else happens.
 * A row's distance depends on the row and its item's F alone, an item's counts on its rows alone: both are bit-identical alone,
 * in any batch, in any slot and for any stride >= counts[b].
 * Null matches / counts / F / dist, batch outside 1..65535, stride < 1, an unknown dtype or kind, a negative or NaN eps, hist
 * without edges or the reverse, nbins < 1 with a histogram or != 0 without -> P2P_EINVAL; nbins > 16 -> P2P_EUNSUPPORTED; all
 * before the device is touched.  No workspace; one launch, one work-group per item (csrc/epipolar.hip), asynchronous on `stream`. */
#define P2P_F32 0
#define P2P_F64 1
#define P2P_I64 2
#define P2P_EPI_SAMPSON  0
#define P2P_EPI_SYM      1
#define P2P_EPI_SYM_SQRT 2
#define P2P_EPI_VALUE    3
int p2p_epipolar_batch(const void *matches, int matches_dtype, const int *counts, const double *F, int batch, int stride,
                       int kind, double eps, const double *edges, int nbins, void *dist, int dist_dtype, int *hist,
                       p2p_stream_t stream);

/* ---- matching operators on their own (since version 110) ------------------------------------------ */

/* The pieces p2p_coarse_forward* fuses, each as an entry point of its own, for callers that build a coarse stage from the
 * reference's operators (networks/modules.py, networks/ncn/model.py, networks/ncn/conv4d.py).  They change nothing above: the fused
 * path keeps its kernels, its limits and its refusals.  Common to all of them: `batch` items contiguous along the leading axis,
 * 1 <= batch <= 65535; one launch (or one per step) for the whole batch; an item's result depends on the item and the sizes
 * alone -- every sum runs in an order the sizes fix -- so it is bit-identical alone, in any batch and in any slot.  Null pointers
 * and non-positive sizes -> P2P_EINVAL, sizes beyond the stated limits -> P2P_EUNSUPPORTED, both before the device is touched. */

/* FeatCorrelation -- reference networks/modules.py:41-53: out[b][pa][pb] = sum_c featA[b][c][pa] * featB[b][c][pb], the plain
 * product: no L2 normalisation, no pooling.
 *   featA [B,C,hA,wA], featB [B,C,hB,wB] -> out [B, hA*wA, hB*wB]   (the reference's '4D' and '3D' shapes are views / permutes)
 * Any C >= 1, any sides >= 1, A and B sizes independent (hA*wA <= 65535 * 64).  Arithmetic: EXACT fp32 on the matrix cores
 * (v_mfma_f32_16x16x4_f32, bit-identical to one fp32 fma chain over the channels in ascending order) -- not the fp16-plane
 * scheme of the fused kernel, whose power-of-two scale relies on normalised features.  csrc/operators.hip. */
int p2p_correlation_batch(const float *featA, const float *featB, int batch, int channels, int hA, int wA, int hB, int wB,
                          float *out, p2p_stream_t stream);

/* maxpool4d -- reference networks/modules.py:11-34 -- of a caller's volume:
 *   x [B,H1,W1,H2,W2] -> pooled_out [B,H1/k,W1/k,H2/k,W2/k] fp32, bit-equal to torch.max over the k^4 slices (a window that
 *   holds a NaN gives NaN and the code of its first NaN, as torch.max does);
 *   delta_out: the same shape, uint8 (optional): s = ((i*k+j)*k+k')*k+l of the FIRST maximum in the reference's slice order
 *   (modules.py:13-18); the unpack kernel above expands it into the reference's four int64 tensors.
 * k: 1 to 4 (k > 4 -> P2P_EUNSUPPORTED: the codes must fit the byte); k = 3 exists here only, the fused coarse entry points keep
 * refusing it.  Sides that are not multiples of k -> P2P_EINVAL.  One thread per pooled cell. */
int p2p_maxpool4d_batch(const float *x, int batch, int h1, int w1, int h2, int w2, int k, float *pooled_out, uint8_t *delta_out,
                        p2p_stream_t stream);

/* MutualMatching -- reference networks/ncn/model.py:157-176 -- in the reference's parenthesisation
 *   y = x * ((x / (maxB + 1e-5)) * (x / (maxA + 1e-5))),   maxB / maxA: the maximum over the B cells of an A cell / over the A cells of a B cell,
 * x [B,hA,wA,hB,wB] -> y_out of the same shape (y_out == x allowed): the maxima and apply kernels of the coarse stage
 * (csrc/coarse.hip section 3; IEEE divisions).  workspace: device memory, 4-byte aligned, the query's bytes (the maxima of every
 * item; P2P_ENOMEM if it is missing or smaller).  The query returns 0 for bad arguments.  Three launches.  hA*wA * hB*wB < 2^31
 * cells per item (the apply kernel indexes in 32 bits; P2P_EUNSUPPORTED beyond). */
size_t p2p_mutual_matching_workspace_bytes(int batch, int hA, int wA, int hB, int wB);
int p2p_mutual_matching_batch(const float *x, int batch, int hA, int wA, int hB, int wB, float *y_out, void *workspace,
                              size_t workspace_bytes, p2p_stream_t stream);

/* One Conv4d layer -- reference networks/ncn/conv4d.py:12-74, 77-130: the "same" 4-D cross-correlation with zero padding k / 2 on
 * all four axes, plus bias; no ReLU.  HOST pointers: weight in the stored (pre-permuted, conv4d.py:119-120) layout
 * [k, c_out, c_in, k, k, k], bias [c_out] or NULL.  c_in, c_out 1..16, kernel_size 3 or 5 (P2P_EUNSUPPORTED otherwise).
 *   x [B,c_in,h1,w1,h2,w2] -> y_out [B,c_out,h1,w1,h2,w2]   (not in place)
 * Arithmetic: exact fp32 on v_mfma_f32_16x16x4_f32, the layer launch of the generic consensus stack (csrc/consensus_generic.hip)
 * reading and writing channel planes.  Every output sums its k^4 c_in terms in an order the layer alone fixes: the K axis (taps
 * outer in the order (da, db, dc, dd), channels inner, c_in padded to 4, 8 or 16 unless it is 1) is cut into super-steps of 16
 * values; super-step S is added, value by value, to partial sum S % 4; the result is (s0 + s1) + (s2 + s3), then + bias.  The four
 * sums keep the rounding error at that of the reference's slice-wise convolutions; a layer of a generic consensus stack keeps ONE
 * chain over the same K order, so a stand-alone layer and the same layer inside such a stack agree to rounding, not bit for bit.
 * Sides may be smaller than the kernel.  Fewer than 2^31 cells. */
typedef struct p2p_conv4d p2p_conv4d;
int p2p_conv4d_create(const float *weight, const float *bias, int c_in, int c_out, int kernel_size, p2p_conv4d **out);
void p2p_conv4d_destroy(p2p_conv4d *conv);
int p2p_conv4d_forward_batch(const p2p_conv4d *conv, const float *x, int batch, int h1, int w1, int h2, int w2, float *y_out,
                             p2p_stream_t stream);

/* L2Normalize -- reference networks/modules.py:6 (eps inside the root): y = x / sqrt(sum_C x^2 + 1e-6) over the middle axis of the
 * contiguous [outer, channels, inner] view of a tensor (dim d of a tensor: outer = the product of the sizes before d, inner = of
 * those after it).  The squares of a position are added in ascending channel order, one fma each; IEEE square root and division.
 * y == x allowed. */
int p2p_l2_normalize(const float *x, size_t outer, int channels, size_t inner, float *y, p2p_stream_t stream);

/* ---- fine stage ------------------------------------------------------------------------------ */

/* One image's feature pyramid levels feat_idx [0,1,2,3] (reference networks/resnet.py:138-157 with
 * change_stride): device pointers [3,H,W], [64,H1,W1], [64,H2,W2], [128,H3,W3] with Hj = ceil(H / 2^j)
 * (the extents the backbone's strided layers produce for ANY H, W -- refine_matches loads images without
 * rounding their size, utils/datasets/preprocess.py:7-30); gathered indices are clamped to H // 2^j - 1 like
 * networks/utils.py:22-23.                                                                     */
typedef struct p2p_pyramid {
    const float *level[4];
    int height, width;      /* of level 0 (the network input); 8 <= H, W < 32768 */
} p2p_pyramid;

/* Patch2Pix.forward_fine_match for one batch item -- reference networks/patch2pix.py:157-218:
 * select_local_patch_feats (networks/utils.py:4-36) -> L2Normalize(dim 0) -> FeatRegressNet
 * (modules.py:101-112) -> parse_regressor_out (patch2pix.py:138-155).
 * With reg2 != NULL the second regressor is run on the first one's output inside the same launch
 * (predict_fine's mid -> fine chain, patch2pix.py:259-272).
 *   proposals   [n,4] int64 (is_float == 0) or fp32 (is_float != 0), device
 *   matches1/probs1 [n,4]/[n] fp32 outputs of reg1 (may be NULL when reg2 != NULL)
 *   matches2/probs2 outputs of reg2 (required when reg2 != NULL)
 *   raw1/raw2   optional [n,5] raw regressor outputs (NULL to skip)
 *   workspace   p2p_regress_workspace_bytes(n) bytes of device memory, 128-byte aligned (scratch of the launch: the pooled
 *               convolution features of every proposal wait there for the batched FC tail; contents are meaningless
 *               outside the call)                                                             */
size_t p2p_regress_workspace_bytes(int n);
/* The same for ONE arithmetic mode (p2p_regress_workspace_bytes is the largest of them = the default mode's):
 * P2P_REGRESS_FP16X2W  4 KB per proposal slot + 512 KiB per proposal of a chunk of at most 3328 (<= 1.74 GB: the value
 *                      jumps from ~2 MB per proposal to that cap once n exceeds one chunk -- callers that run another
 *                      mode should size their buffer with this query, not with p2p_regress_workspace_bytes),
 * P2P_REGRESS_FP16     the same with 256 KiB per proposal of a chunk (never more than P2P_REGRESS_FP16X2W),
 * P2P_REGRESS_FP16X2   4 KB per proposal slot,   P2P_REGRESS_F32   0 (the buffer is ignored).                      */
size_t p2p_regress_workspace_bytes_mode(int n, int mode);
/* The same for ONE handle.  Tuned handles: the value of p2p_regress_workspace_bytes_mode for the handle's mode.  Generic
 * handles: the scratch of one chunk of min(n, 256) proposals rounded up to whole units of 8, per proposal
 *   4 (mid matches) + fc_in (pooled features) + 2 max(fc_dim) + the largest activation a layer reads + the largest it writes
 * floats, activations counted as spp x h x w x channels (spp = 2 samples per proposal for 'post', 1 for 'pre'; layer 0
 * reads 16 x 16 x the selected channels padded to a multiple of 8).  Released configuration: 669 712 bytes per proposal,
 * 171 MB at the cap of 256.  The value depends on the handle's mode: P2P_REGRESS_GENERIC_FP16X2 adds spp x (n_conv - 1)
 * floats per proposal, the per-sample words its inner layers derive their input scales from (released configuration: 4
 * bytes per proposal more) -- query again after p2p_regressor_set_mode.  p2p_regress* derive their chunk from the workspace_bytes they are given -- the largest
 * multiple of 8 proposals that fits, at most the cap -- and return P2P_ENOMEM below one unit of 8; results do not depend
 * on the chunk.                                                                                                     */
size_t p2p_regress_workspace_bytes_for(const p2p_regressor *reg, int n);
int p2p_regress(const p2p_regressor *reg1, const p2p_regressor *reg2,
                const p2p_pyramid *im1, const p2p_pyramid *im2,
                const void *proposals, int is_float, int n,
                float *matches1, float *probs1, float *raw1,
                float *matches2, float *probs2, float *raw2,
                void *workspace, size_t workspace_bytes, p2p_stream_t stream);

/* The same for `nitems` image pairs in one launch (the reference loops over the batch items of its
 * list arguments, patch2pix.py:192): im1/im2 are arrays of nitems pyramids, counts[i] (HOST array) the
 * number of proposals of item i; proposals and every output are the per-item arrays concatenated in
 * item order.  Filling the chip matters here: one proposal occupies one compute unit.  workspace:
 * p2p_regress_workspace_bytes(sum of counts).                                                   */
int p2p_regress_batch(const p2p_regressor *reg1, const p2p_regressor *reg2, int nitems,
                      const p2p_pyramid *im1, const p2p_pyramid *im2, const int *counts,
                      const void *proposals, int is_float,
                      float *matches1, float *probs1, float *raw1,
                      float *matches2, float *probs2, float *raw2,
                      void *workspace, size_t workspace_bytes, p2p_stream_t stream);

/* The same with the proposal counts in DEVICE memory (e.g. written by p2p_filter_coarse_batch): every item owns
 * `stride` slots of the proposal and output arrays ([nitems*stride, ...]), of which the first dev_counts[i] are used;
 * the other slots' outputs are left untouched.  Nothing has to come back to the host between the coarse and the fine
 * stage.  workspace: p2p_regress_workspace_bytes(nitems * stride).                                                 */
int p2p_regress_batch_dev(const p2p_regressor *reg1, const p2p_regressor *reg2, int nitems,
                          const p2p_pyramid *im1, const p2p_pyramid *im2, const int *dev_counts, int stride,
                          const void *proposals, int is_float,
                          float *matches1, float *probs1, float *raw1,
                          float *matches2, float *probs2, float *raw2,
                          void *workspace, size_t workspace_bytes, p2p_stream_t stream);

/* ---- feature-pyramid producer (the convolutions of ResNet34 / 50 / 101 layer1..layer3) ------- */

/* One Conv2d(ci, co, ks, stride, padding = ks / 2, bias = False) + BatchNorm2d(co) in eval mode -- reference
 * networks/resnet.py:26-100 (BasicBlock: conv1/bn1, conv2/bn2, downsample; Bottleneck: conv1..conv3, downsample) as used by
 * forward_all (:138-157) with or without the layer3 stride patch (:169-173).  HOST pointers: weight [co,ci,ks,ks], the four
 * BatchNorm vectors [co].  Supported: ks 1 or 3, stride 1 or 2, ci a multiple of 32, co a multiple of 64 (of 128 at stride 2):
 * every convolution of layer1..layer3 of the three backbones, up to 1024 channels on either side.
 * Arithmetic: fp32-equivalent (operands as two fp16 planes under exact power-of-two scales, three MFMA products per
 * fp32 product, fp32 accumulation).                                                                             */
typedef struct p2p_conv p2p_conv;
int p2p_conv_create(const float *weight, const p2p_bn_params *bn, int ci, int co, int ks, int stride, p2p_conv **out);
void p2p_conv_destroy(p2p_conv *conv);
/* Experiments / tests: force the work-group tile (mt, nt, wn) of this layer's launches -- [32 mt (4 / wn) pixels] x
 * [32 nt wn channels]; (0,0,0) = chosen from the launch size (default).  A tile the layer does not have is ignored.  The
 * result does not depend on the tile (every tile sums an output's K axis in the same order).                          */
int p2p_conv_set_tile(p2p_conv *conv, int mt, int nt, int wn);
/* The arithmetic of this handle's launches (since version 112).  P2P_CONV_FP16X2 is the default described above.
 * P2P_CONV_FP16 is opt-in and NOT fp32-equivalent: the same kernels with ONE fp16 plane per operand (the fp16 rounding of
 * the activation and of the weight under the same exact power-of-two scales: relative operand rounding 2^-11) and one MFMA
 * product per fp32 product; scales, fp32 accumulation, epilogue, tiles and ymax are the default's.  Both modes read the one
 * packed weight blob, so a mode change uploads nothing and p2p_conv_set_tile works in both.  Features computed in this mode
 * move the correlation volume: coarse match indices can differ from the default mode's at near-ties, and the mode is not
 * held to the index / 1e-3 px bars of the other paths.  An unknown mode is P2P_EINVAL.                              */
#define P2P_CONV_FP16X2 0
#define P2P_CONV_FP16   1
int p2p_conv_set_mode(p2p_conv *conv, int mode);
int p2p_conv_get_mode(const p2p_conv *conv);

/* y = [relu](bn(conv(x)) [+ residual]) for a batch of n images.  Activations are fp32 **NHWC** device arrays
 * (x [n,h,w,ci], y and residual [n,ho,wo,co], ho = (h + 2 (ks/2) - ks) / stride + 1); xmax [n] holds the float bits of
 * max |x| per image (p2p_absmax_batch, or the ymax of the producing call); ymax (optional, [n] int, **zero on entry**:
 * the kernel raises it with atomicMax) receives the same for y.  The three steps of a BasicBlock: conv1 (relu = 1), downsample (relu = 0, when present), conv2 (residual =
 * the block input or the downsample output, relu = 1).                                                           */
int p2p_conv_forward(const p2p_conv *conv, const float *x, const int *xmax, int n, int h, int w, const float *residual,
                     int relu, float *y, int *ymax, p2p_stream_t stream);

/* The stem: Conv2d(3, 64, 7, stride 2, padding 3, bias = False) + BatchNorm2d(64) + ReLU -- reference
 * networks/resnet.py:101-103 as used at :141-143.  HOST pointers: weight [64,3,7,7] + BatchNorm vectors.  image [n,3,h,w]
 * NCHW fp32 (device), imax [n] float bits of max |image| per item; y [n,64,ho,wo] **NCHW** (pyramid level 1 as the fine
 * stage reads it), ho = (h - 1) / 2 + 1.                                                                         */
typedef struct p2p_stem p2p_stem;
int p2p_stem_create(const float *weight, const p2p_bn_params *bn, p2p_stem **out);
void p2p_stem_destroy(p2p_stem *stem);
/* P2P_CONV_FP16X2 (default) / P2P_CONV_FP16, as p2p_conv_set_mode (since version 112).                              */
int p2p_stem_set_mode(p2p_stem *stem, int mode);
int p2p_stem_get_mode(const p2p_stem *stem);
int p2p_stem_forward(const p2p_stem *stem, const float *image, const int *imax, int n, int h, int w, float *y, p2p_stream_t stream);

/* MaxPool2d(kernel 3, stride 2, padding 1) -- reference networks/resnet.py:104,146: x [n,c,h,w] NCHW -> y [n,hp,wp,c]
 * **NHWC** (hp = (h - 1) / 2 + 1), the input layout of p2p_conv_forward; ymax (optional, zero on entry) as there.  c a multiple of 64. */
int p2p_maxpool_nhwc(const float *x, int n, int c, int h, int w, float *y, int *ymax, p2p_stream_t stream);

/* [n,h,w,c] -> [n,c,h,w]: a pyramid level in the layout p2p_coarse_forward / p2p_regress read.                     */
int p2p_nhwc_to_nchw(const float *x, int n, int h, int w, int c, float *y, p2p_stream_t stream);

/* out[i] = float bits of max |x| over the count values of item i (items are count values apart).                 */
int p2p_absmax_batch(const float *x, size_t count, int items, int *out, p2p_stream_t stream);

/* ---- image preprocessing (since version 107) --------------------------------------------------- */

/* Pillow's Image.resize(size, Image.BICUBIC) for 8-bit RGB (default box, no reducing_gap), BIT FOR BIT, optionally fused with
 * the /255, -mean, /std normalisation -- reference utils/datasets/preprocess.py:32-60 (load_im_flexible) from the decoded
 * pixels on.  csrc/preprocess.hip: a horizontal pass into a uint8 intermediate image, then a vertical pass, in Pillow's
 * fixed-point arithmetic (coefficients with 22 fractional bits, int32 accumulator starting at 2^21, clip8(acc >> 22)).
 *
 * The library computes no coefficient: per axis whose size changes the caller provides a TABLE in DEVICE memory, int32,
 *   bounds [out][2]      (first input coordinate, number of taps n <= ksize) per output coordinate, then
 *   coeffs [out][ksize]  the n fixed-point coefficients of that coordinate, zero beyond n,
 * with ksize = (int)ceil(2 * max(in / out, 1)) * 2 + 1 in double arithmetic, computed on the host the way Pillow's
 * precompute_coeffs + normalize_coeffs_8bpc do (patch2pix_amd.utils.datasets.preprocess.resize_tables is that computation;
 * the Python layer uploads the tables through its ring of pinned buffers).  One table serves every item of that (in, out)
 * pair.  An axis that keeps its size has a NULL table and is copied.  ksize_x / ksize_y are checked against the sizes
 * (P2P_EINVAL); windows are clamped to the image on the device, so a malformed table gives wrong pixels, never a fault.
 * With Pillow's tables the first window starts at 0 and the last one ends at `in`: the horizontal pass covers all in_h rows,
 * which are exactly the rows the vertical pass reads.
 *
 *   items      HOST array of `batch` descriptors: pixels = DEVICE pointer to uint8 [in_h, in_w, 3]; every item its own size
 *   out_u8     optional, device: uint8 [batch, out_h, out_w, 3]
 *   out_f32    optional, device: item i is written as float32 [3, out_h, out_w] at out_f32 + i * out_f32_stride (floats;
 *              >= 3 out_h out_w -- a slot range of a larger [B,3,H,W] tensor), value lut[c * 256 + byte]; lut: device
 *              float32 [3,256], required with out_f32.  At least one of the two outputs.
 *   workspace  p2p_resize_workspace_bytes(batch, largest in_h, largest in_w, out_h, out_w) bytes of device memory, 16-byte
 *              aligned: the intermediate images (in_h rows of out_w pixels at a 16-byte pitch per item).  It does NOT hold the
 *              tables (they are the caller's, see above).  May be NULL when no item changes its width.
 * Limits: every side 1..16384; a width ratio in_w / out_w up to 2048 (P2P_EUNSUPPORTED beyond: the taps of one output pixel
 * and the input segment they read are staged in 64 KiB of LDS) -- this covers every input side up to 8192 with every output
 * side from 4 up, above the input side (upscaling) included.  Null pointers and sizes <= 0 -> P2P_EINVAL, a workspace that is
 * missing or too small -> P2P_ENOMEM, both before the device is touched.  Nothing is allocated; two launches per 64 items,
 * asynchronous on `stream`.  The query returns 0 for bad arguments.                                                    */
typedef struct p2p_resize_item {
    const uint8_t *pixels;
    int in_h, in_w;
    const int32_t *table_x, *table_y;      /* in_w -> out_w, in_h -> out_h; NULL where the size stays */
    int ksize_x, ksize_y;                  /* ignored for a NULL table */
} p2p_resize_item;
size_t p2p_resize_workspace_bytes(int batch, int max_in_h, int max_in_w, int out_h, int out_w);
int p2p_resize_bicubic_batch(const p2p_resize_item *items, int batch, int out_h, int out_w, uint8_t *out_u8, float *out_f32,
                             size_t out_f32_stride, const float *lut, void *workspace, size_t workspace_bytes,
                             p2p_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* P2P_HIP_H */
