// Coarse stage of the Patch2Pix matching path on gfx950 (reference networks/patch2pix.py:120-136,
// :340-375): L2-normalise -> 4-D correlation -> 4-D max-pool -> mutual matching -> neighbourhood
// consensus (two 3^4 convolutions, symmetric) -> mutual matching -> soft mutual-NN matches.
//
// Data layout in HBM (A = image 1 cells, B = image 2 cells):
//   Fn      [row block of 128 pos'][K chunk of 32 ch][plane 2][row 128][4 pieces of 8 ch] fp16: L2-normalised layer-3
//                         features x 2^12 as two fp16 planes (one plane in mode P2P_COARSE_FP16: blocks of half the size), in the 16 KB blocks the correlation GEMM copies into LDS by
//                         LDS-DMA (piece q of row r at slot q ^ ((r >> 2) & 3): conflict-free fragment reads); positions
//                         re-ordered cell-major so that the k^2 positions of one pooling cell are adjacent:
//                         pos' = cell*k^2 + (i%k)*k + (j%k)  (k = 4: image A's rows permuted once more inside blocks of
//                         32, prep_row_k4)
//   P, Y, Y2 [nA'][nB']   fp32 pooled correlation volume viewed as a matrix (row = A cell, col = B cell); Y / Y2 =
//                         the two branches of the consensus net (consensus.hip), summed by the kernels that read them
//   delta   [nA'][nB']    uint8 argmax code s = ((di*k+dj)*k+dk)*k+dl
// The full-resolution correlation (92 MB at 480x640, 1.5 GB at 960x1280) is never written: the
// pooling runs on the MFMA accumulators of the correlation GEMM; the 16-channel hidden volume of the
// consensus net never leaves LDS.  ONE arithmetic whatever the batch (fp32-equivalent fp16x2 on the matrix
// cores, fp32 elsewhere): a pair's results do not depend on the pairs it shares a launch with.
//
// Batches: the reference's tensors carry a batch axis ([B,C,h,w] features of B equally sized pairs).  Every
// kernel takes the pair from blockIdx.z and a per-pair stride for each of its pointers, so a batch is
// ONE launch per kernel (B x the work-groups: the 30x40x30x40 volume of a single 480x640 pair does not
// fill 256 CUs in the consensus layers).
//
// This file: sections 1-3, each kernel with its launcher.  4, the neighbourhood consensus (ncn/model.py:145-155; conv4d.py:12-74):
// consensus.hip (the released stack, one fused kernel) and consensus_generic.hip (any other); 5, matches.hip; 6, the pair score
// (patch2pix.py:320-338): score.hip; host API: coarse_api.hip.
#include "coarse_common.h"

namespace p2p {

constexpr float MM_EPS = 1e-5f;

// monotone float <-> int key so that atomicMax(int) implements a float max (order independent)
__device__ __forceinline__ int f2key(float f) {
    int b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float key2f(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }
constexpr int KEY_NEG_INF = (int)0xff800000 ^ 0x7fffffff;

// ------------------------------------------------------------------------------------------------
// 1. L2 normalise + transpose to position-major with cell-major position order (modules.py:6)
// ------------------------------------------------------------------------------------------------
constexpr int PREP_P = 16;    // positions per work-group (300 groups at 60x80: fills the chip)
// Writes the normalised features x 2^12 as two fp16 planes (|v| <= 1, so both planes stay in the normal range of fp16 and
// v * 2^12 = p0 + p1 to within 2^-24 |v * 2^12|) in the block layout of the correlation GEMM (CX_BLK, below).
constexpr float CORR_FP16_SCALE = 4096.0f;
// One launch for both images of every pair (blockIdx.y = image); the same launch resets the maxima keys of the mutual
// matchings (nkeys words = -inf, then one word = 0: the float bits of max |X|, see mm_apply_kernel).
// k = 4: a pooling cell is 16 GEMM rows (image A) x 16 GEMM columns (image B).  The rows of image A are permuted inside
// every block of 32 (= two cells) so that cell e of the block sits on the rows (q & 3) + 8 (q >> 2) + 4 e, q = di * 4 + dj:
// the rows whose products one half e of a wave holds in its 32x32 accumulator block, in register order (corr_pool_kernel<4>).
__device__ __forceinline__ int prep_row_k4(int pp) { return (pp & ~31) + (pp & 3) + 2 * (pp & 12) + ((pp >> 2) & 4); }
// (PERM_A = the k = 4 instantiation: a template parameter, so that the kernel of k = 1, 2 is the code it was without it)
// NP = planes per operand: 2 = the fp32-equivalent split (default), 1 = the single-plane mode P2P_COARSE_FP16 -- the first plane
// alone (one rounding to fp16, 2^-11 relative), in blocks of half the size: [row 128][4 pieces of 8 ch] = 8 KB per K chunk.
// WIDE: the tile of C > 256 channels (the 512 / 1024 of a Bottleneck backbone) lives in dynamic LDS sized by C (68 KB at 1024:
// two work-groups per compute unit); C <= 256 keeps the static 17 KB tile and is the instantiation it always was, so its buffers
// keep their bits.  The code is the same: the whole channel column of a position is resident, so the sum of squares stays ONE
// fixed-order fp32 reduction per position (16 strided partial sums in ascending channel order, then their sum in ascending group
// order) whatever C, batch and tiling.
constexpr int PREP_C_STATIC = 256, PREP_C_MAX = 1024;
template <bool PERM_A, int NP = 2, bool WIDE = false>
__global__ __launch_bounds__(256) void prep_kernel(PrepArgs a) {
    const int img = blockIdx.y;
    if (img == 0) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i <= a.nkeys) a.keys[blockIdx.z * a.sKeys + i] = (i < a.nkeys) ? KEY_NEG_INF : 0;
    }
    const int h = a.h[img], w = a.w[img], C = a.C, k = a.k;
    const bool perm = PERM_A && img == 0;
    if ((int)blockIdx.x * PREP_P >= h * w) return;
    const float *__restrict__ F = a.F[img] + blockIdx.z * a.sF[img];
    unsigned short *__restrict__ Fn = a.Fn[img] + blockIdx.z * a.sFn;
    // The GEMM copies whole 128-row blocks: the rows between h * w and the next multiple of 128 are zeros, never uninitialised
    // memory (its stores are masked, so their products were never used -- but NaN bit patterns went through the matrix cores).
    // The work-group of the last positions writes them: <= 127 rows x C channels x 2 planes, 16 bytes per store.
    if (((int)blockIdx.x + 1) * PREP_P >= h * w) {
        const int pad0 = h * w, pad1 = (pad0 + 127) & ~127, pieces = (C >> 5) * NP * 4;      // 16-byte pieces per row
        for (int e = threadIdx.x; e < (pad1 - pad0) * pieces; e += 256) {
            const int pr = pad0 + e / pieces;
            const int r = (perm ? prep_row_k4(pr) : pr) & 127, q = e % pieces, kc = q / (NP * 4), pl = (q >> 2) & (NP - 1), piece = q & 3;
            unsigned short *d = Fn + ((size_t)(pad0 >> 7) * (C >> 5) + kc) * (NP * 128 * 32) + pl * (128 * 32) + (r * 4 + piece) * 8;
            *(f32x4 *)d = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
    __shared__ float tile_static[(WIDE ? 1 : PREP_C_STATIC) * (PREP_P + 1)];   // [C <= 256][17]
    float *tile = tile_static;
    if constexpr (WIDE) {
        P2P_DYN_SHARED(float, tile_wide);                                      // [C <= 1024][17]
        tile = tile_wide;
    }
    __shared__ float part[16][PREP_P];
    __shared__ float inv[PREP_P];
    const int hw = h * w;
    const int p0 = blockIdx.x * PREP_P;
    const int tid = threadIdx.x;
    // 4 threads x float4 cover the 16 positions of one channel row (64 contiguous bytes)
    for (int e = tid; e < C * 4; e += 256) {
        const int c = e >> 2, q = e & 3;
        const int pos = p0 + 4 * q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (pos + 3 < hw && (hw & 3) == 0) v = *(const f32x4 *)(F + (size_t)c * hw + pos);
        else
            for (int i = 0; i < 4; ++i) if (pos + i < hw) v[i] = F[(size_t)c * hw + pos + i];
        float *t = tile + c * (PREP_P + 1) + 4 * q;
        t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
    }
    __syncthreads();
    {   // sum of squares: 16 channel groups x 16 positions, ascending channel order within a group
        const int p = tid & 15, g = tid >> 4;
        float ss = 0.f;
        for (int c = g; c < C; c += 16) { const float v = tile[c * (PREP_P + 1) + p]; ss = fmaf(v, v, ss); }
        part[g][p] = ss;
    }
    __syncthreads();
    if (tid < PREP_P) {
        float ss = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) ss += part[g][tid];
        inv[tid] = 1.0f / sqrtf(ss + 1e-6f);
    }
    __syncthreads();
    const int wc = w / k;
    for (int p = 0; p < PREP_P; ++p) {
        const int pos = p0 + p;
        if (pos >= hw) break;
        const int i = pos / w, j = pos - i * w;
        int pp = ((i / k) * wc + (j / k)) * (k * k) + (i % k) * k + (j % k);
        if (perm) pp = prep_row_k4(pp);
        for (int c = tid; c < C; c += 256) {
            const float x = tile[c * (PREP_P + 1) + p] * inv[p] * CORR_FP16_SCALE;
            // block (pp / 128, c / 32): [plane][row pp % 128][piece (c / 8) % 4 at slot piece ^ ((row / 4) % 4)][c % 8]
            const int r = pp & 127;
            unsigned short *d = Fn + ((size_t)(pp >> 7) * (C >> 5) + (c >> 5)) * (NP * 128 * 32) +
                                (r * 4 + (((c >> 3) & 3) ^ ((r >> 2) & 3))) * 8 + (c & 7);
            const _Float16 h0 = (_Float16)x;
            d[0] = __builtin_bit_cast(unsigned short, h0);
            if constexpr (NP == 2) d[128 * 32] = __builtin_bit_cast(unsigned short, (_Float16)(x - (float)h0));
        }
    }
}

int launch_prep(const PrepArgs &a, int planes, unsigned nz, hipStream_t stream) {
    const int gp = std::max(ceil_div(std::max(a.h[0] * a.w[0], a.h[1] * a.w[1]), PREP_P), ceil_div(a.nkeys + 1, 256));
    if (a.C > PREP_C_STATIC) {
        if (a.C > PREP_C_MAX) {
            set_error("launch_prep: %d channels (at most %d)", a.C, PREP_C_MAX);
            return P2P_EUNSUPPORTED;
        }
        constexpr int lds_max = PREP_C_MAX * (PREP_P + 1) * (int)sizeof(float);
        static DeviceOnce attr_set;
        const int dev = raise_lds_limit(attr_set, {{(const void *)prep_kernel<true, 1, true>, lds_max}, {(const void *)prep_kernel<false, 1, true>, lds_max},
                                                   {(const void *)prep_kernel<true, 2, true>, lds_max}, {(const void *)prep_kernel<false, 2, true>, lds_max}});
        if (dev < 0) return dev;
        const auto kernel = planes == 1 ? (a.k == 4 ? prep_kernel<true, 1, true> : prep_kernel<false, 1, true>)
                                        : (a.k == 4 ? prep_kernel<true, 2, true> : prep_kernel<false, 2, true>);
        hipLaunchKernelGGL(kernel, dim3(gp, 2, nz), dim3(256), (size_t)a.C * (PREP_P + 1) * sizeof(float), stream, a);
        return P2P_OK;
    }
    const auto kernel = planes == 1 ? (a.k == 4 ? prep_kernel<true, 1> : prep_kernel<false, 1>)
                                    : (a.k == 4 ? prep_kernel<true, 2> : prep_kernel<false, 2>);
    hipLaunchKernelGGL(kernel, dim3(gp, 2, nz), dim3(256), 0, stream, a);
    return P2P_OK;
}

// ------------------------------------------------------------------------------------------------
// 2. correlation GEMM (modules.py:41-53) with the 4-D max-pool (modules.py:11-34) in the epilogue
//    C[pA'][pB'] = sum_c FnA[pA'][c] * FnB[pB'][c];  128x128 tile, 4 waves x (2x2) tiles of 32x32
// ------------------------------------------------------------------------------------------------
// fp32-equivalent arithmetic on the fp16 matrix cores: both operands arrive as two fp16 planes of the features times 2^12
// (prep_kernel), three v_mfma_f32_32x32x16_f16 per product (a0 b0 + a0 b1 + a1 b0; the dropped a1 b1 is <= 2^-24 of the
// product), the accumulators are scaled back by 2^-24 (exact) in the epilogue.  fp32 accumulation, no VALU in the loop: per
// K = 16 slab and wave 8 ds_read_b128 and 12 MFMAs.
// Staging (round 5): the operands of a K = 32 stage are two 16 KB blocks that prep_kernel wrote as the LDS image, copied by
// LDS-DMA (global_load_lds_dwordx4: no VGPR round trip, no ds_write_b128 -- the store path of the register-staged version
// took more LDS cycles than the fragment reads) into a double buffer: the DMA of stage i + 1 is in flight while stage i is
// multiplied, one vmcnt(0) + raw s_barrier per stage; the fragments of slab s + 1 are read behind the MFMAs of slab s.
// LDS: [stage 2][A|B][plane 2][128 rows][4 pieces of 16 B, XOR-swizzled] = 64 KB, two work-groups per compute unit.
//
// Tile order.  The hardware deals consecutive work-group ids to the 8 XCDs round-robin, and every XCD has its own 4 MB L2.
// A row-major raster therefore makes every XCD stream ALL B panels for every row of tiles (960x1280: 3.1 GB fetched per
// pair for 39 MB of operands).  Here work-group id g belongs to XCD g % 8, and XCD x walks the x-th eighth of a
// "block-major" order: blocks of CX_AB tile rows (their A panels, CX_AB x 128 KB, stay in the L2), inside a block column
// after column of B tiles -- each B panel is fetched once per block instead of once per tile row.
constexpr int CT = 128;      // tile edge
constexpr int CX_AB = 16;    // tile rows per L2-resident block of A panels (16 x 128 KB = 2 MB of the 4 MB L2; measured at
                             // 960x1280: 16 rows fetch 224 MB per pair, 24 rows 246 MB, 28 rows 682 MB -- the streaming B
                             // panels and the output need the other half)
typedef _Float16 cf16x8 __attribute__((ext_vector_type(8)));
// Sizes per plane count NP (corr_pool_kernel defines CX_BLK = cx_blk(NP), CX_STAGE = 2 CX_BLK for the macros below)
constexpr int cx_blk(int np) { return np * CT * 64; }       // one operand block of a stage: [plane NP][row 128][32 K fp16] = 16 KB (NP = 2)
constexpr int cx_lds(int np) { return 4 * cx_blk(np); }     // [stage 2][A|B] blocks
__device__ __forceinline__ f32x16 cx_mfma(const f32x4 &a, const f32x4 &b, const f32x16 &c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cf16x8, a), __builtin_bit_cast(cf16x8, b), c, 0, 0, 0);
}
// stage IT of the tile -> ring slot SLOT: wave w copies bytes [CX_BLK / 4 w, CX_BLK / 4 (w + 1)) of the A and of the B block
// (4096 bytes = four copies per block with two planes, 2048 = two with one)
#define CX_ISSUE(IT, SLOT)                                                                                             \
    {                                                                                                                  \
        const unsigned char *ga_ = Ab + (size_t)(IT) * CX_BLK + lane16;                                                \
        const unsigned char *gb_ = Bb + (size_t)(IT) * CX_BLK + lane16;                                                \
        unsigned char *la_ = cx + (SLOT) * CX_STAGE + wave * (CX_BLK / 4);                                             \
        P2P_GLOBAL_LOAD_LDS16(ga_, la_, 0); P2P_GLOBAL_LOAD_LDS16(ga_, la_, 1024);                                     \
        if constexpr (NP == 2) { P2P_GLOBAL_LOAD_LDS16(ga_, la_, 2048); P2P_GLOBAL_LOAD_LDS16(ga_, la_, 3072); }       \
        P2P_GLOBAL_LOAD_LDS16(gb_, la_ + CX_BLK, 0); P2P_GLOBAL_LOAD_LDS16(gb_, la_ + CX_BLK, 1024);                   \
        if constexpr (NP == 2) { P2P_GLOBAL_LOAD_LDS16(gb_, la_ + CX_BLK, 2048); P2P_GLOBAL_LOAD_LDS16(gb_, la_ + CX_BLK, 3072); } \
    }
// fragments of slab S of ring slot SLOT: a[m-tile][plane], b[n-tile][plane]
#define CX_READ(FA, FB, SLOT, S)                                                                                       \
    {                                                                                                                  \
        const unsigned char *pa_ = cx + (SLOT) * CX_STAGE + ((S) ? aoff1 : aoff0);                                     \
        const unsigned char *pb_ = cx + (SLOT) * CX_STAGE + CX_BLK + ((S) ? boff1 : boff0);                            \
        _Pragma("unroll") for (int t_ = 0; t_ < 2; ++t_)                                                               \
            _Pragma("unroll") for (int q_ = 0; q_ < NP; ++q_) {                                                        \
                FA[t_][q_] = *(const f32x4 *)(pa_ + t_ * 2048 + q_ * 8192);                                            \
                FB[t_][q_] = *(const f32x4 *)(pb_ + t_ * 2048 + q_ * 8192);                                            \
            }                                                                                                          \
    }
// smallest terms first (a1 b0, a0 b1, a0 b0); the four accumulators rotate.  One plane: a0 b0 alone
#define CX_SLAB(FA, FB)                                                                                                \
    _Pragma("unroll") for (int t_ = (NP == 2 ? 0 : 2); t_ < 3; ++t_) {                                                 \
        const int pa_ = (t_ == 0) ? 1 : 0, pb_ = (t_ == 1) ? 1 : 0;                                                    \
        _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_)                                                               \
            _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_) acc[i_][j_] = cx_mfma(FA[i_][pa_], FB[j_][pb_], acc[i_][j_]); \
    }
// one LDS read behind each of the first eight MFMAs of a slab (left alone the compiler builds read -> wait -> MFMA chains);
// one plane: a slab is four MFMAs and the next slab's four reads
#define CX_PIPE()                                                                                                      \
    _Pragma("unroll") for (int g_ = 0; g_ < 4 * NP; ++g_) {                                                            \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }        \
    if constexpr (NP == 2) __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                                          \
    __builtin_amdgcn_sched_barrier(0);

// WIDE (C > 256): the matrix cores add into an accumulator chain of 6 (NP = 2) products per stage, and the error of that chain
// grows with its length (measured at 1024 channels: the volume 2.5 - 4.5 x as far from fp64 as an fp32 GEMM's, against 1.5 x at
// 256).  Every CX_FLUSH stages the accumulators are therefore added (VALU fp32, round to nearest) into a second set and start
// again from zero: chains of at most CX_FLUSH stages whatever C, their sums added in ascending K order -- the same fixed order
// for every tile, pair and batch.  C <= 256 is the instantiation without the second set: its arithmetic and bits are unchanged.
constexpr int CX_FLUSH = 4;
template <int KS, int NP = 2, bool WIDE = false>
__global__ __launch_bounds__(256, 2) void corr_pool_kernel(const unsigned short *__restrict__ A, const unsigned short *__restrict__ B,
                                                           int nA, int nB, int C, float *__restrict__ P,
                                                           uint8_t *__restrict__ delta, size_t sAB, size_t sP, size_t sDelta,
                                                           int gx, int gy, int ntiles, int per_xcd) {
    // Persistent work-groups: XCD x = blockIdx.x % 8 owns the tiles [x * per_xcd, (x + 1) * per_xcd) of the order described
    // under "Tile order", its work-group j = blockIdx.x / 8 walks j, j + G, j + 2G, ... of them (G work-groups per XCD);
    // stage 0 of the next tile is in flight during the pooling epilogue of the current one.
    constexpr int CX_BLK = cx_blk(NP), CX_STAGE = 2 * CX_BLK;
    const int Gx = gridDim.x >> 3, xcd = blockIdx.x & 7;
    int tj = blockIdx.x >> 3;
    // tile number -> (pair, A tile row, B tile column)
    int rowA0 = 0, rowB0 = 0, zp = 0;
    const unsigned char *Ab = nullptr, *Bb = nullptr;             // the tile's first blocks: stage it = block it of the row block
    auto locate = [&](int j, int &ra, int &rb, int &z, const unsigned char *&pa, const unsigned char *&pb) -> bool {
        const int L = xcd * per_xcd + j;
        if (j >= per_xcd || L >= ntiles) return false;
        const int tp = gx * gy;
        z = L / tp;
        const int r = L - z * tp;
        const int blk = r / (CX_AB * gx), rr = r - blk * (CX_AB * gx);
        const int hb = min(CX_AB, gy - blk * CX_AB);
        const int bcol = rr / hb, arow = blk * CX_AB + rr - bcol * hb;
        ra = arow * CT; rb = bcol * CT;
        pa = (const unsigned char *)(A + (size_t)z * sAB) + (size_t)arow * (C >> 5) * CX_BLK;
        pb = (const unsigned char *)(B + (size_t)z * sAB) + (size_t)bcol * (C >> 5) * CX_BLK;
        return true;
    };
    if (!locate(tj, rowA0, rowB0, zp, Ab, Bb)) return;
    P2P_DYN_SHARED(unsigned char, cx);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int half = lane >> 5, l31 = lane & 31;
    const unsigned lane16 = wave * (CX_BLK / 4) + lane * 16;
    // fragment addresses inside a block: row r, piece (2 slab + half) ^ ((r >> 2) & 3)
    const int sw = (l31 >> 2) & 3;
    const unsigned aoff0 = ((wr * 64 + l31) * 4 + ((0 + half) ^ sw)) * 16, aoff1 = ((wr * 64 + l31) * 4 + ((2 + half) ^ sw)) * 16;
    const unsigned boff0 = ((wc * 64 + l31) * 4 + ((0 + half) ^ sw)) * 16, boff1 = ((wc * 64 + l31) * 4 + ((2 + half) ^ sw)) * 16;

    const int nk = C / 32;
    CX_ISSUE(0, 0)
#pragma unroll 1
  for (;;) {
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x16){0};

    f32x16 tot[WIDE ? 2 : 1][WIDE ? 2 : 1];
    if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) tot[i][j] = (f32x16){0};
    }
    f32x4 xa[2][NP], xb[2][NP], ya[2][NP], yb[2][NP];
#pragma unroll 1
    for (int it = 0; it < nk; it += 2) {
        if constexpr (WIDE) {
            if (it && (it & (CX_FLUSH - 1)) == 0) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) { tot[i][j] += acc[i][j]; acc[i][j] = (f32x16){0}; }
            }
        }
        // even stage (slot 0): its pieces have landed for everybody behind the barrier, and everybody is done with slot 1
        P2P_WAIT_VMCNT(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (it + 1 < nk) CX_ISSUE(it + 1, 1)
        CX_READ(xa, xb, 0, 0)
        __builtin_amdgcn_sched_barrier(0);
        CX_READ(ya, yb, 0, 1)
        CX_SLAB(xa, xb)
        CX_PIPE()
        CX_SLAB(ya, yb)
        __builtin_amdgcn_sched_barrier(0);
        if (it + 1 >= nk) break;
        // odd stage (slot 1)
        P2P_WAIT_VMCNT(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (it + 2 < nk) CX_ISSUE(it + 2, 0)
        CX_READ(xa, xb, 1, 0)
        __builtin_amdgcn_sched_barrier(0);
        CX_READ(ya, yb, 1, 1)
        CX_SLAB(xa, xb)
        CX_PIPE()
        CX_SLAB(ya, yb)
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = tot[i][j] + acc[i][j];
    }
    // the next tile of this work-group: its stage 0 goes to slot 0 behind a barrier (everybody is done reading the ring)
    const int rowA0c = rowA0, rowB0c = rowB0;
    float *Pz = P + (size_t)zp * sP;
    uint8_t *dz = delta ? delta + (size_t)zp * sDelta : nullptr;
    tj += Gx;
    const bool more = locate(tj, rowA0, rowB0, zp, Ab, Bb);
    __builtin_amdgcn_s_barrier();
    if (more) CX_ISSUE(0, 0)
    __builtin_amdgcn_sched_barrier(0);
    // the planes carried 2^12 each: the accumulators hold 2^24 x the correlation (undone exactly at the stores; a maximum
    // commutes with the positive power of two)
    constexpr float inv = 1.0f / (CORR_FP16_SCALE * CORR_FP16_SCALE);

    // accumulator element r of lane: row = (r&3) + 8*(r>>2) + 4*half, col = l31
    if (KS == 1) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int tr = rowA0c + wr * 64 + i * 32, tc = rowB0c + wc * 64 + j * 32;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = tr + (r & 3) + 8 * (r >> 2) + 4 * half, col = tc + l31;
                    if (row < nA && col < nB) Pz[(size_t)row * nB + col] = acc[i][j][r] * inv;
                }
            }
    } else if (KS == 2)
    // k = 2: a pooling cell is a 4x4 block: rows = (i,j) of A in regs 4g..4g+3, cols = (k,l) of B in 4 adjacent lanes.
    // First maximum in the order s = row_in_cell*4 + col_in_cell.  The exchange inside a quad of lanes is two DPP moves per
    // value (quad_perm; __shfl_xor goes through the LDS crossbar and is waited for: 64 of them were a third of a tile's
    // time), the pooled offsets are 32-bit (a pooled volume has < 2^31 cells), the bounds of a tile are checked once.
    {
        const int nAc = nA >> 2, nBc = nB >> 2;
        const int crow0 = ((rowA0c + wr * 64) >> 2) + half, ccol0 = (rowB0c + wc * 64 + l31) >> 2;
        const bool writer = (lane & 3) == 0;
        const bool full = ((rowA0c + CT) >> 2) <= nAc && ((rowB0c + CT) >> 2) <= nBc;      // (wave-uniform) no cell of the tile is outside
        // all sixteen cells of the lane's quad first (the exchanges need every lane), then ONE masked block of stores
        float pbest[2][2][4];
        int ps[2][2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float best = acc[i][j][4 * g];
                    int s = 0;
#pragma unroll
                    for (int r = 1; r < 4; ++r) {
                        const float v = acc[i][j][4 * g + r];
                        if (v > best) { best = v; s = r; }
                    }
                    s = s * 4 + (lane & 3);
                    {
                        const float ov = __uint_as_float(P2P_SWAP_ADJACENT(__float_as_uint(best)));
                        const int os = (int)P2P_SWAP_ADJACENT((unsigned)s);
                        if (ov > best || (ov == best && os < s)) { best = ov; s = os; }
                    }
                    {
                        const float ov = __uint_as_float(P2P_SWAP_PAIRS(__float_as_uint(best)));
                        const int os = (int)P2P_SWAP_PAIRS((unsigned)s);
                        if (ov > best || (ov == best && os < s)) { best = ov; s = os; }
                    }
                    pbest[i][j][g] = best * inv;
                    ps[i][j][g] = s;
                }
        if (writer) {
            float *Pl = Pz + (unsigned)(crow0 * nBc + ccol0);
            uint8_t *Dl = dz ? dz + (unsigned)(crow0 * nBc + ccol0) : nullptr;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int dr = 8 * i + 2 * g, dc = 8 * j;
                        if (full || (crow0 + dr < nAc && ccol0 + dc < nBc)) {
                            const unsigned at = (unsigned)(dr * nBc + dc);
                            Pl[at] = pbest[i][j][g];
                            if (Dl) Dl[at] = (uint8_t)ps[i][j][g];
                        }
                    }
        }
    }
    if (KS == 4) {
        // k = 4: a 32x32 accumulator block holds 2x2 cells.  prep_kernel put the 16 positions (di, dj) of an A cell on the
        // rows of ONE half of the wave in register order (prep_row_k4), so register r of a lane is (di, dj) = (r >> 2, r & 3)
        // of cell row `half`, and the 16 columns (dk, dl) of a B cell are the 16 lanes of a DPP row: the first maximum of the
        // lane's own registers, then four DPP exchanges (lane ^ 1, ^ 2, ^ 7, ^ 8 span the row) under the total order
        // "larger value, then smaller s" -- every lane of the row ends with the cell's result, lane 0 of it stores.
        const int nAc = nA >> 4, nBc = nB >> 4;
        const int crow0 = ((rowA0c + wr * 64) >> 4) + half, ccol0 = (rowB0c + wc * 64 + l31) >> 4;
        float pbest[2][2];
        int ps[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float best = acc[i][j][0];
                int s = 0;
#pragma unroll
                for (int r = 1; r < 16; ++r) {
                    const float v = acc[i][j][r];
                    if (v > best) { best = v; s = r; }
                }
                s = s * 16 + (lane & 15);
#define CX_K4_STEP(XCHG)                                                                                               \
                {                                                                                                      \
                    const float ov = __uint_as_float(XCHG(__float_as_uint(best)));                                     \
                    const int os = (int)XCHG((unsigned)s);                                                             \
                    if (ov > best || (ov == best && os < s)) { best = ov; s = os; }                                    \
                }
                CX_K4_STEP(P2P_SWAP_ADJACENT)
                CX_K4_STEP(P2P_SWAP_PAIRS)
                CX_K4_STEP(P2P_MIRROR_HALF_ROW)
                CX_K4_STEP(P2P_SWAP_HALF_ROWS)
#undef CX_K4_STEP
                pbest[i][j] = best * inv;
                ps[i][j] = s;
            }
        if ((lane & 15) == 0) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int cr = crow0 + 2 * i, cc = ccol0 + 2 * j;
                    if (cr < nAc && cc < nBc) {          // the padding rows of a tile are whole cells of zeros: never stored
                        const unsigned at = (unsigned)(cr * nBc + cc);
                        Pz[at] = pbest[i][j];
                        if (dz) dz[at] = (uint8_t)ps[i][j];
                    }
                }
        }
    }
    if (!more) break;
  }
}

int launch_corr_pool(const unsigned short *fnA, const unsigned short *fnB, int nA, int nB, int C, int ksize, int planes, float *P,
                     uint8_t *delta, size_t sAB, size_t sP, size_t sDelta, unsigned nz, hipStream_t stream) {
    static DeviceOnce attr_set_dev;      // per device: a process may drive several GPUs
    const int dev = raise_lds_limit(attr_set_dev, {{(const void *)corr_pool_kernel<1, 2>, cx_lds(2)}, {(const void *)corr_pool_kernel<2, 2>, cx_lds(2)},
                                                   {(const void *)corr_pool_kernel<4, 2>, cx_lds(2)}, {(const void *)corr_pool_kernel<1, 1>, cx_lds(1)},
                                                   {(const void *)corr_pool_kernel<2, 1>, cx_lds(1)}, {(const void *)corr_pool_kernel<4, 1>, cx_lds(1)},
                                                   {(const void *)corr_pool_kernel<1, 2, true>, cx_lds(2)}, {(const void *)corr_pool_kernel<2, 2, true>, cx_lds(2)},
                                                   {(const void *)corr_pool_kernel<4, 2, true>, cx_lds(2)}, {(const void *)corr_pool_kernel<1, 1, true>, cx_lds(1)},
                                                   {(const void *)corr_pool_kernel<2, 1, true>, cx_lds(1)}, {(const void *)corr_pool_kernel<4, 1, true>, cx_lds(1)}});
    if (dev < 0) return dev;
    const int gx = ceil_div(nB, CT), gy = ceil_div(nA, CT);
    const long long ntiles = (long long)gx * gy * nz;
    P2P_REQUIRE(ntiles < (1ll << 30), P2P_EUNSUPPORTED, "p2p_coarse_forward: %lld correlation tiles in one launch", ntiles);
    // persistent work-groups: two fit a compute unit, 32 compute units per XCD
    const int per_xcd = (int)((ntiles + 7) / 8);
    const dim3 cgrid((unsigned)(8 * std::min(per_xcd, 64)));
    if (ksize == 1) delta = nullptr, sDelta = 0;       // nothing was pooled: no argmax to record
    const auto kernel = C > 256
        ? (planes == 1 ? (ksize == 1 ? corr_pool_kernel<1, 1, true> : (ksize == 4 ? corr_pool_kernel<4, 1, true> : corr_pool_kernel<2, 1, true>))
                       : (ksize == 1 ? corr_pool_kernel<1, 2, true> : (ksize == 4 ? corr_pool_kernel<4, 2, true> : corr_pool_kernel<2, 2, true>)))
        : (planes == 1 ? (ksize == 1 ? corr_pool_kernel<1, 1> : (ksize == 4 ? corr_pool_kernel<4, 1> : corr_pool_kernel<2, 1>))
                       : (ksize == 1 ? corr_pool_kernel<1, 2> : (ksize == 4 ? corr_pool_kernel<4, 2> : corr_pool_kernel<2, 2>)));
    hipLaunchKernelGGL(kernel, cgrid, dim3(256), cx_lds(planes), stream, fnA, fnB, nA, nB, C, P, delta, sAB, sP, sDelta, gx, gy, (int)ntiles, per_xcd);
    return P2P_OK;
}

// ------------------------------------------------------------------------------------------------
// 3. row / column maxima of an [nA][nB] matrix (the two torch.max of ncn/model.py:165-166)
// ------------------------------------------------------------------------------------------------
// One launch for both: the first gridDim.x - ceil(nA / 4) work-groups take the column maxima (a thread owns one column
// over a 64-row chunk; chunks meet in an order independent atomicMax), the others the row maxima (one wave per row).
// (X2: optional second addend of every value -- the fused consensus kernel leaves its two branches in two arrays)
__global__ __launch_bounds__(256) void maxima_kernel(const float *__restrict__ X, int nA, int nB, int *rkey, int *ckey, size_t sX,
                                                     size_t sKeys, const float *__restrict__ X2, int col_groups) {
    X += blockIdx.z * sX;
    if (X2) X2 += blockIdx.z * sX;
    rkey += blockIdx.z * sKeys;
    ckey += blockIdx.z * sKeys;
    const int gcol = (nB + 255) / 256;
    if ((int)blockIdx.x < col_groups) {
        const int col = ((int)blockIdx.x % gcol) * 256 + threadIdx.x;
        if (col >= nB) return;
        const int r0 = ((int)blockIdx.x / gcol) * 64, r1 = min(r0 + 64, nA);
        float cm = -INFINITY;
        if (X2) {
#pragma unroll 8
            for (int r = r0; r < r1; ++r) cm = fmaxf(cm, X[(size_t)r * nB + col] + X2[(size_t)r * nB + col]);
        } else {
#pragma unroll 8
            for (int r = r0; r < r1; ++r) cm = fmaxf(cm, X[(size_t)r * nB + col]);
        }
        atomicMax(&ckey[col], f2key(cm));
        return;
    }
    const int row = ((int)blockIdx.x - col_groups) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= nA) return;
    const float *x = X + (size_t)row * nB;
    float rm = -INFINITY;
    if (X2) {
        const float *x2 = X2 + (size_t)row * nB;
        for (int c = lane; c < nB; c += 64) rm = fmaxf(rm, x[c] + x2[c]);
    } else {
        for (int c = lane; c < nB; c += 64) rm = fmaxf(rm, x[c]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) rm = fmaxf(rm, __shfl_xor(rm, m));
    if (lane == 0) rkey[row] = f2key(rm);
}

void launch_maxima(const float *X, int nA, int nB, int *rkey, int *ckey, size_t sX, size_t sKeys, const float *X2, unsigned nz,
                   hipStream_t stream) {
    const int col_groups = ceil_div(nB, 256) * ceil_div(nA, 64);
    const dim3 grid(col_groups + ceil_div(nA, 4), 1, nz);
    hipLaunchKernelGGL(maxima_kernel, grid, dim3(256), 0, stream, X, nA, nB, rkey, ckey, sX, sKeys, X2, col_groups);
}

// MutualMatching value (ncn/model.py:168-175): x * ((x / (max_over_B + eps)) * (x / (max_over_A + eps)))
__device__ __forceinline__ float mm_value(float x, float max_over_b, float max_over_a) {
    const float xa = x / (max_over_b + MM_EPS);
    const float xb = x / (max_over_a + MM_EPS);
    return x * (xa * xb);
}

// (in place when out == X).  VEC: a thread owns four adjacent columns of a row (one 16-byte load and store per array); the
// scalar form is for volumes whose rows are not a multiple of four cells.  The divisions stay IEEE divisions (the values
// must round like the reference's); the index split is one 32-bit division per thread.
typedef int mm_i32x4 __attribute__((ext_vector_type(4)));
template <bool VEC>
__global__ __launch_bounds__(256) void mm_apply_kernel(const float *X, int nA, int nB, const int *__restrict__ rkey,
                                                       const int *__restrict__ ckey, float *out, size_t sX, size_t sKeys,
                                                       size_t sOut, int *amax, const float *X2) {
    X += blockIdx.z * sX;
    if (X2) X2 += blockIdx.z * sX;
    rkey += blockIdx.z * sKeys;
    ckey += blockIdx.z * sKeys;
    out += blockIdx.z * sOut;
    constexpr int V = VEC ? 4 : 1;
    const unsigned per_row = (unsigned)nB / V;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    float m = 0.f;
    if (i < (unsigned)nA * per_row) {
        const unsigned r = i / per_row, c = (i - r * per_row) * V;
        const size_t at = (size_t)r * nB + c;
        const float mb = key2f(rkey[r]);
        if constexpr (VEC) {
            f32x4 x = *(const f32x4 *)(X + at);
            if (X2) {
                const f32x4 y = *(const f32x4 *)(X2 + at);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] += y[j];
            }
            const mm_i32x4 ck = *(const mm_i32x4 *)(ckey + c);
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = mm_value(x[j], mb, key2f(ck[j]));
                m = fmaxf(m, fabsf(v[j]));
            }
            *(f32x4 *)(out + at) = v;
        } else {
            const float v = mm_value(X2 ? X[at] + X2[at] : X[at], mb, key2f(ckey[c]));
            out[at] = v;
            m = fabsf(v);
        }
    }
    if (amax) {                                     // largest magnitude of the volume (the fused consensus kernel scales its fp16 planes by it)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
        // the word only grows: a (possibly stale) plain read first keeps nearly every wave off the atomic unit
        int *dst = amax + blockIdx.z * sKeys;
        if ((threadIdx.x & 63) == 0 && __float_as_int(m) > *(volatile int *)dst) atomicMax(dst, __float_as_int(m));
    }
}

void launch_mm_apply(const float *X, int nA, int nB, const int *rkey, const int *ckey, float *out, size_t sX, size_t sKeys,
                     size_t sOut, int *amax, const float *X2, size_t nz, hipStream_t stream) {
    const bool vec = nB % 4 == 0 && sX % 4 == 0 && sOut % 4 == 0 && sKeys % 4 == 0 && ((uintptr_t)X & 15) == 0 &&
                     ((uintptr_t)out & 15) == 0 && ((uintptr_t)X2 & 15) == 0 && ((uintptr_t)ckey & 15) == 0;
    const size_t items = (size_t)nA * (nB / (vec ? 4 : 1));
    const dim3 grid((unsigned)((items + 255) / 256), 1, (unsigned)nz);
    if (vec) hipLaunchKernelGGL(mm_apply_kernel<true>, grid, dim3(256), 0, stream, X, nA, nB, rkey, ckey, out, sX, sKeys, sOut, amax, X2);
    else hipLaunchKernelGGL(mm_apply_kernel<false>, grid, dim3(256), 0, stream, X, nA, nB, rkey, ckey, out, sX, sKeys, sOut, amax, X2);
}

}  // namespace p2p

// sections 4 (its shape-generic part), 5 and 6, and the stand-alone operators: no units of their own
#include "consensus_generic.hip"
#include "consensus_generic_h2.hip"
#include "matches.hip"
#include "score.hip"
#include "operators.hip"
