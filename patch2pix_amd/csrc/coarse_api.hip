// Coarse stage, host side: the p2p_ncn handle (the fused kernel's packed weights in a DeviceBlob, host_pack.h, or a generic stack), the carve-up of the caller's
// workspace, and the p2p_coarse_* / p2p_neigh_consensus_* / p2p_delta_unpack entry points of include/p2p_hip.h.  No kernel lives
// here and none is launched from here: every kernel sits next to its launcher (coarse.hip, matches.hip, score.hip, consensus.hip,
// consensus_generic.hip; declared in coarse_common.h).  Compiled as part of api.hip, not as a unit of its own.
#include "coarse_common.h"

using namespace p2p;

// workspace carve-up shared by the size query and the launcher
struct CoarseWs {
    size_t fnA, fnB, P, Y, Y2, keys, act, total;   // byte offsets
};
// gen: the generic consensus net whose activation buffers the pair's block holds as well (null: a tuned handle, none)
static CoarseWs coarse_ws(int C, int hA, int wA, int hB, int wB, int k, const NcGen *gen = nullptr, int mode = 0) {
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t nA = (size_t)hA * wA, nB = (size_t)hB * wB;
    const size_t nAc = nA / (k * k), nBc = nB / (k * k);
    CoarseWs w;
    size_t off = 0;
    w.fnA = off; off += al(((nA + 127) / 128) * 128 * C * 4);      // two fp16 planes in blocks of 128 positions x 32 channels
    w.fnB = off; off += al(((nB + 127) / 128) * 128 * C * 4);
    w.P = off; off += al(nAc * nBc * 4);
    w.Y = off; off += al(nAc * nBc * 4);     // the two branches of the consensus net
    w.Y2 = off; off += al(nAc * nBc * 4);
    w.keys = off; off += al((2 * (nAc + nBc) + 1) * 4);      // row / column maxima of both mutual matchings + max |X|
    w.act = off;
    if (gen) off += nc_generic_ws_bytes(*gen, nAc * nBc, mode);
    w.total = off;
    return w;
}

extern "C" int p2p_ncn_create(const float *w1, const float *b1, const float *w2, const float *b2, p2p_ncn **out) {
    P2P_REQUIRE(w1 && b1 && w2 && b2 && out, P2P_EINVAL, "p2p_ncn_create: null argument");
    // stored layout (conv4d.py:119-120): w1s[da][o][ci=0][db][dc][dd], w2s[da][o=0][ci][db][dc][dd] -> MFMA fragments of
    // both branches (consensus.hip)
    DeviceBlob wf;
    pack_nc_fused(w1, b1, w2, wf);
    const int st = wf.upload("p2p_ncn_create: the consensus weights");
    if (st != P2P_OK) return st;
    *out = new p2p_ncn{b2[0], std::move(wf), {0, 0, 0}, nullptr};
    return P2P_OK;
}

extern "C" int p2p_ncn_create_config(const p2p_ncn_config *config, const p2p_ncn_tensors *tensors, p2p_ncn **out) {
    P2P_REQUIRE(out, P2P_EINVAL, "p2p_ncn_create_config: null argument");
    NcGen *g = nullptr;
    const int st = nc_generic_create(config, tensors, &g);      // validates before it touches the device
    if (st != P2P_OK) return st;
    *out = new p2p_ncn{0.f, DeviceBlob(), {0, 0, 0}, g};
    return P2P_OK;
}

extern "C" int p2p_ncn_is_generic(const p2p_ncn *ncn) { return ncn ? (ncn->gen ? 1 : 0) : -1; }

extern "C" int p2p_ncn_set_tile(p2p_ncn *ncn, int ta, int tb, int tc) {
    P2P_REQUIRE(ncn && ta >= 0 && tb >= 0 && tc >= 0, P2P_EINVAL, "p2p_ncn_set_tile: bad argument");
    P2P_REQUIRE(!ncn->gen, P2P_EUNSUPPORTED, "p2p_ncn_set_tile: a generic consensus handle has no work-group tile to force");
    // (0, 0, 0) = automatic; (ta, tb, tc) with tb, tc > 0 = forced (ta = 0: only the march length is picked); anything else
    // would be ignored silently
    P2P_REQUIRE((tb > 0 && tc > 0) || (ta == 0 && tb == 0 && tc == 0), P2P_EINVAL,
                "p2p_ncn_set_tile: (%d, %d, %d) is neither (0, 0, 0) nor a tile with tb, tc > 0", ta, tb, tc);
    ncn->tile[0] = ta; ncn->tile[1] = tb; ncn->tile[2] = tc;
    return P2P_OK;
}

extern "C" int p2p_ncn_set_mode(p2p_ncn *ncn, int mode) {
    P2P_REQUIRE(ncn, P2P_EINVAL, "p2p_ncn_set_mode: null handle");
    P2P_REQUIRE(mode == P2P_COARSE_FP16X2 || mode == P2P_COARSE_FP16 || mode == P2P_COARSE_GENERIC_FP16X2, P2P_EINVAL,
                "p2p_ncn_set_mode: unknown mode %d", mode);
    if (mode == P2P_COARSE_GENERIC_FP16X2) {
        P2P_REQUIRE(ncn->gen, P2P_EUNSUPPORTED, "p2p_ncn_set_mode: P2P_COARSE_GENERIC_FP16X2 is a mode of generic consensus handles");
        const int st = nc_generic_ensure_h2(ncn->gen);      // packs and uploads the planes on the first selection
        if (st != P2P_OK) return st;
    }
    // 0 is every handle's default arithmetic: exact fp32 for a generic one
    P2P_REQUIRE(!ncn->gen || mode != P2P_COARSE_FP16, P2P_EUNSUPPORTED,
                "p2p_ncn_set_mode: a generic consensus handle has no single-plane mode (0 or P2P_COARSE_GENERIC_FP16X2)");
    ncn->mode = mode;
    return P2P_OK;
}

extern "C" int p2p_ncn_get_mode(const p2p_ncn *ncn) { return ncn ? ncn->mode : -1; }

// fp16 planes per operand of the handle's mode
static int coarse_planes(const p2p_ncn *ncn) { return ncn->mode == P2P_COARSE_FP16 ? 1 : 2; }

extern "C" void p2p_ncn_destroy(p2p_ncn *ncn) { delete ncn; }

extern "C" size_t p2p_coarse_workspace_bytes(int channels, int hA, int wA, int hB, int wB, int ksize) {
    if (channels <= 0 || hA <= 0 || wA <= 0 || hB <= 0 || wB <= 0 || ksize < 1) return 0;
    return coarse_ws(channels, hA, wA, hB, wB, ksize).total;
}

extern "C" size_t p2p_coarse_workspace_bytes_for(const p2p_ncn *ncn, int channels, int hA, int wA, int hB, int wB, int ksize) {
    if (!ncn || channels <= 0 || hA <= 0 || wA <= 0 || hB <= 0 || wB <= 0 || ksize < 1) return 0;
    return coarse_ws(channels, hA, wA, hB, wB, ksize, ncn->gen, ncn->mode).total;
}

extern "C" size_t p2p_neigh_consensus_workspace_bytes(const p2p_ncn *ncn, int hA, int wA, int hB, int wB) {
    if (!ncn || hA <= 0 || wA <= 0 || hB <= 0 || wB <= 0) return 0;
    return ncn->gen ? nc_generic_ws_bytes(*ncn->gen, (size_t)hA * wA * hB * wB, ncn->mode) : sizeof(int);
}

extern "C" int p2p_coarse_forward_batch(const float *featA, const float *featB, int batch, int C, int hA, int wA, int hB,
                                        int wB, int ksize, const p2p_ncn *ncn, float *corr4d_out, uint8_t *delta_out,
                                        void *workspace, size_t workspace_bytes, p2p_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    P2P_REQUIRE(featA && featB && ncn && corr4d_out && workspace, P2P_EINVAL, "p2p_coarse_forward: null argument");
    P2P_REQUIRE(batch >= 1 && batch <= 65535, P2P_EINVAL, "p2p_coarse_forward: batch %d out of range", batch);
    P2P_REQUIRE(ksize == 1 || ksize == 2 || ksize == 4, P2P_EUNSUPPORTED, "p2p_coarse_forward: ksize %d not supported (1, 2 or 4)", ksize);
    P2P_REQUIRE(C > 0 && C % 32 == 0 && C <= 1024, P2P_EUNSUPPORTED, "p2p_coarse_forward: channels %d (multiple of 32, <= 1024)", C);
    P2P_REQUIRE(hA > 0 && wA > 0 && hB > 0 && wB > 0 && hA % ksize == 0 && wA % ksize == 0 && hB % ksize == 0 &&
                    wB % ksize == 0, P2P_EINVAL, "p2p_coarse_forward: feature map sizes must be positive multiples of ksize");
    // The handle is dereferenced only after the workspace has passed the size every kind of handle needs: callers probe this
    // entry point's argument checks with placeholder handles (tests/test_cabi_exports.py::test_batch_argument_errors passes
    // ncn = 1 with a 64-byte workspace and expects the workspace error, as before generic handles existed).
    const size_t ws_any = coarse_ws(C, hA, wA, hB, wB, ksize).total;
    P2P_REQUIRE(workspace_bytes >= ws_any, P2P_ENOMEM, "p2p_coarse_forward: workspace %zu < %zu bytes (one pair)", workspace_bytes, ws_any);
    const CoarseWs ws = coarse_ws(C, hA, wA, hB, wB, ksize, ncn->gen, ncn->mode);
    P2P_REQUIRE(workspace_bytes >= ws.total, P2P_ENOMEM, "p2p_coarse_forward: workspace %zu < %zu bytes (one pair)", workspace_bytes,
                ws.total);
    P2P_REQUIRE(!ncn->gen || ((uintptr_t)workspace & 15) == 0, P2P_EINVAL,
                "p2p_coarse_forward: the workspace of a generic handle must be 16-byte aligned");
    const int nA = hA * wA, nB = hB * wB, kk = ksize * ksize;
    const int nAc = nA / kk, nBc = nB / kk;
    const size_t nel = (size_t)nAc * nBc;
    const size_t sWs = ws.total / 4;        // every workspace buffer of pair z sits z * ws.total bytes further on
    const int per_launch = (int)std::min<size_t>(batch, workspace_bytes / ws.total);   // pairs the workspace holds at once
    const int d0 = hA / ksize, d1 = wA / ksize, d2 = hB / ksize, d3 = wB / ksize;
    const int planes = coarse_planes(ncn);      // one plane: the feature blocks fill the first half of their (two-plane sized) buffers
    for (int z0 = 0; z0 < batch; z0 += per_launch) {
        const unsigned nz = (unsigned)std::min(per_launch, batch - z0);
        const float *fA = featA + (size_t)z0 * C * nA, *fB = featB + (size_t)z0 * C * nB;
        float *out = corr4d_out + (size_t)z0 * nel;
        uint8_t *dout = delta_out ? delta_out + (size_t)z0 * nel : nullptr;
        char *base = (char *)workspace;
        unsigned short *fnA = (unsigned short *)(base + ws.fnA), *fnB = (unsigned short *)(base + ws.fnB);
        float *P = (float *)(base + ws.P), *Y = (float *)(base + ws.Y), *Y2 = (float *)(base + ws.Y2);
        int *rkey1 = (int *)(base + ws.keys), *ckey1 = rkey1 + nAc, *rkey2 = ckey1 + nBc, *ckey2 = rkey2 + nAc;
        const int nkeys = 2 * (nAc + nBc);
        int *xmax = rkey1 + nkeys;
        int st = launch_prep(PrepArgs{{fA, fB}, {fnA, fnB}, {hA, hB}, {wA, wB}, {(size_t)C * nA, (size_t)C * nB}, C, ksize, 2 * sWs, rkey1, nkeys, sWs},
                             planes, nz, stream);
        if (st != P2P_OK) return st;
        st = launch_corr_pool(fnA, fnB, nA, nB, C, ksize, planes, P, dout, 2 * sWs, sWs, nel, nz, stream);
        if (st != P2P_OK) return st;
        launch_maxima(P, nAc, nBc, rkey1, ckey1, sWs, sWs, nullptr, nz, stream);
        // first mutual matching, in place on the pooled volume (+ max |X| for the consensus kernel's operand scale)
        launch_mm_apply(P, nAc, nBc, rkey1, ckey1, P, sWs, sWs, sWs, xmax, nullptr, nz, stream);
        if (ncn->gen) {   // a generic stack: layer by layer, the sum of its branches in Y
            st = launch_nc_generic(*ncn->gen, ncn->mode, P, sWs, Y, sWs, (float *)(base + ws.act), sWs, (int)nz, d0, d1, d2, d3, stream);
            Y2 = nullptr;
        } else {   // both consensus layers, both branches: relu(.) of the direct branch into Y, of the transposed one into Y2
            st = launch_nc_fused(P, Y, Y2, sWs, (int)nz, d0, d1, d2, d3, ncn->wfused.dev<unsigned char>(), ncn->b2, xmax, sWs, ncn->tile, planes, stream);
        }
        if (st != P2P_OK) return st;
        launch_maxima(Y, nAc, nBc, rkey2, ckey2, sWs, sWs, Y2, nz, stream);
        launch_mm_apply(Y, nAc, nBc, rkey2, ckey2, out, sWs, sWs, nel, nullptr, Y2, nz, stream);
    }
    return check_launch("coarse_forward kernels");
}

extern "C" int p2p_coarse_forward(const float *featA, const float *featB, int C, int hA, int wA, int hB, int wB,
                                  int ksize, const p2p_ncn *ncn, float *corr4d_out, uint8_t *delta_out,
                                  void *workspace, size_t workspace_bytes, p2p_stream_t stream) {
    return p2p_coarse_forward_batch(featA, featB, 1, C, hA, wA, hB, wB, ksize, ncn, corr4d_out, delta_out, workspace,
                                    workspace_bytes, stream);
}

extern "C" int p2p_neigh_consensus_batch(const float *x, int batch, int hA, int wA, int hB, int wB, const p2p_ncn *ncn, float *y_out,
                                         void *workspace, size_t workspace_bytes, p2p_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    P2P_REQUIRE(x && ncn && y_out && workspace, P2P_EINVAL, "p2p_neigh_consensus: null argument");
    P2P_REQUIRE(batch >= 1 && batch <= 65535 && hA > 0 && wA > 0 && hB > 0 && wB > 0, P2P_EINVAL, "p2p_neigh_consensus: bad sizes");
    if (ncn->gen) {
        const size_t cells = (size_t)hA * wA * hB * wB, per = nc_generic_ws_bytes(*ncn->gen, cells, ncn->mode);
        P2P_REQUIRE(workspace_bytes >= per, P2P_ENOMEM, "p2p_neigh_consensus: workspace %zu < %zu bytes (one volume)", workspace_bytes, per);
        P2P_REQUIRE(((uintptr_t)workspace & 15) == 0, P2P_EINVAL, "p2p_neigh_consensus: the workspace of a generic handle must be 16-byte aligned");
        const int per_launch = (int)std::min<size_t>(batch, workspace_bytes / per);      // volumes the workspace holds at once
        for (int z0 = 0; z0 < batch; z0 += per_launch) {
            const int st = launch_nc_generic(*ncn->gen, ncn->mode, x + (size_t)z0 * cells, cells, y_out + (size_t)z0 * cells, cells, (float *)workspace,
                                             per / sizeof(float), std::min(per_launch, batch - z0), hA, wA, hB, wB, stream);
            if (st != P2P_OK) return st;
        }
        return P2P_OK;
    }
    P2P_REQUIRE(workspace_bytes >= (size_t)batch * sizeof(int), P2P_ENOMEM, "p2p_neigh_consensus: workspace of %zu bytes needed (4 per volume)",
                (size_t)batch * sizeof(int));
    const size_t nel = (size_t)hA * wA * hB * wB;
    int *xmax = (int *)workspace;
    P2P_HIP_CHECK(hipMemsetAsync(y_out, 0, (size_t)batch * nel * sizeof(float), stream));
    P2P_HIP_CHECK(hipMemsetAsync(xmax, 0, (size_t)batch * sizeof(int), stream));
    const int st = launch_absmax(x, nel, nel, batch, xmax, 1, stream);
    if (st != P2P_OK) return st;
    return launch_nc_fused(x, y_out, nullptr, nel, batch, hA, wA, hB, wB, ncn->wfused.dev<unsigned char>(), ncn->b2, xmax, 1, ncn->tile, coarse_planes(ncn), stream);
}

extern "C" int p2p_delta_unpack(const uint8_t *delta, size_t n, int ksize, int64_t *out, p2p_stream_t stream) {
    P2P_REQUIRE(delta && out && ksize >= 1, P2P_EINVAL, "p2p_delta_unpack: bad argument");
    if (n == 0) return P2P_OK;
    launch_delta_unpack(delta, n, ksize, (long long *)out, (hipStream_t)stream);
    return check_launch("delta_unpack_kernel");
}

// what the two match entry points check alike (fn: the name their messages start with)
static int check_match_args(const char *fn, const float *corr4d, const uint8_t *delta, int batch, int hA, int wA, int hB, int wB,
                            int ksize, const int64_t *matches_out, const float *scores_out) {
    P2P_REQUIRE(corr4d && matches_out && scores_out, P2P_EINVAL, "%s: null argument", fn);
    P2P_REQUIRE(batch >= 1 && batch <= 65535, P2P_EINVAL, "%s: batch %d out of range", fn, batch);
    P2P_REQUIRE(hA > 0 && wA > 0 && hB > 0 && wB > 0 && ksize >= 1, P2P_EINVAL, "%s: bad sizes", fn);
    P2P_REQUIRE(ksize == 1 || delta, P2P_EINVAL, "%s: delta required when ksize > 1", fn);
    return P2P_OK;
}

extern "C" int p2p_coarse_matches_batch(const float *corr4d, const uint8_t *delta, int batch, int hA, int wA, int hB, int wB,
                                        int ksize, int upsample, int center, int64_t *matches_out, float *scores_out,
                                        p2p_stream_t stream) {
    const int st = check_match_args("p2p_coarse_matches", corr4d, delta, batch, hA, wA, hB, wB, ksize, matches_out, scores_out);
    if (st != P2P_OK) return st;
    const int nA = hA * wA, nB = hB * wB;
    MatchArgs m{corr4d, delta, hA, wA, hB, wB, ksize, upsample, center, (long long *)matches_out, scores_out,
                (size_t)nA * nB, (size_t)nA + nB};
    launch_matches(m, batch, (hipStream_t)stream);
    return check_launch("match kernels");
}

extern "C" int p2p_coarse_matches_topk_batch(const float *corr4d, const uint8_t *delta, int batch, int hA, int wA, int hB, int wB,
                                             int ksize, int upsample, int center, int topk, int do_softmax,
                                             int64_t *matches_out, float *scores_out, p2p_stream_t stream) {
    const int st = check_match_args("p2p_coarse_matches_topk", corr4d, delta, batch, hA, wA, hB, wB, ksize, matches_out, scores_out);
    if (st != P2P_OK) return st;
    const int nA = hA * wA, nB = hB * wB;
    P2P_REQUIRE(topk >= 1 && topk <= 8, P2P_EINVAL, "p2p_coarse_matches_topk: topk %d out of range (1 to 8)", topk);
    P2P_REQUIRE(topk <= std::min(nA, nB), P2P_EINVAL, "p2p_coarse_matches_topk: topk %d exceeds the %d cells of an image", topk,
                std::min(nA, nB));
    MatchArgs m{corr4d, delta, hA, wA, hB, wB, ksize, upsample, center, (long long *)matches_out, scores_out,
                (size_t)nA * nB, (size_t)topk * ((size_t)nA + nB)};
    launch_matches_topk(m, batch, topk, do_softmax ? 1 : 0, (hipStream_t)stream);
    return check_launch("top-k match kernels");
}

extern "C" size_t p2p_coarse_score_workspace_bytes(int batch, int hA, int wA, int hB, int wB) {
    if (batch < 1 || batch > 65535 || hA <= 0 || wA <= 0 || hB <= 0 || wB <= 0) return 0;
    return (size_t)batch * ((size_t)hA * wA + (size_t)hB * wB) * sizeof(float);
}

extern "C" int p2p_coarse_score_batch(const float *corr4d, int batch, int hA, int wA, int hB, int wB, int normalize,
                                      float *cell_scores, float *pair_scores, void *workspace, size_t workspace_bytes,
                                      p2p_stream_t stream) {
    P2P_REQUIRE(corr4d && pair_scores, P2P_EINVAL, "p2p_coarse_score: null argument");
    P2P_REQUIRE(batch >= 1 && batch <= 65535, P2P_EINVAL, "p2p_coarse_score: batch %d out of range", batch);
    P2P_REQUIRE(hA > 0 && wA > 0 && hB > 0 && wB > 0, P2P_EINVAL, "p2p_coarse_score: bad sizes");
    const long long nA = (long long)hA * wA, nB = (long long)hB * wB;
    P2P_REQUIRE(nA + nB < (1ll << 30), P2P_EINVAL, "p2p_coarse_score: bad sizes (%lld + %lld cells)", nA, nB);
    P2P_REQUIRE(normalize == P2P_SCORE_NONE || normalize == P2P_SCORE_SOFTMAX || normalize == P2P_SCORE_L1, P2P_EINVAL,
                "p2p_coarse_score: unknown normalisation %d", normalize);
    if (!cell_scores) {      // the cell scores wait in the caller's scratch for the pair kernel
        const size_t need = p2p_coarse_score_workspace_bytes(batch, hA, wA, hB, wB);
        P2P_REQUIRE(workspace && workspace_bytes >= need, P2P_ENOMEM, "p2p_coarse_score: workspace of %zu bytes needed without cell_scores",
                    need);
        P2P_REQUIRE(((uintptr_t)workspace & 3) == 0, P2P_EINVAL, "p2p_coarse_score: the workspace must be 4-byte aligned");
        cell_scores = (float *)workspace;
    }
    launch_score(ScoreArgs{corr4d, cell_scores, pair_scores, (int)nA, (int)nB, (size_t)(nA * nB)}, batch, normalize, (hipStream_t)stream);
    return check_launch("score kernels");
}

extern "C" int p2p_coarse_matches(const float *corr4d, const uint8_t *delta, int hA, int wA, int hB, int wB, int ksize,
                                  int upsample, int center, int64_t *matches_out, float *scores_out, p2p_stream_t stream) {
    return p2p_coarse_matches_batch(corr4d, delta, 1, hA, wA, hB, wB, ksize, upsample, center, matches_out, scores_out, stream);
}
