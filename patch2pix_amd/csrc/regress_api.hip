// Fine stage, host side: the regressor handle (one RegDev view and one DeviceBlob, host_pack.h, per arithmetic mode, plus the blob
// of the parameters every mode shares), mode selection, the p2p_regress* entry points and the workspace queries of include/p2p_hip.h.  No kernel lives here: a mode is a row of MODES, whose launcher and
// packers sit next to their kernels (regress.hip, regress_h2.hip, regress_wino.hip; declared in regress_common.h).  Compiled
// as part of api.hip, not as a unit of its own.
#include "regress_common.h"
#include "regress_generic.hip"      // the shape-generic kernels and their handle (generic regressors; no unit of its own either)
#include "regress_generic_h2.hip"   // their fp16x2 convolution stack (mode P2P_REGRESS_GENERIC_FP16X2)

using namespace p2p;

// Arithmetic of the two convolutions: new regressors start in P2P_REGRESS_DEFAULT, p2p_regressor_set_mode selects another
// mode per handle (the library reads no environment variables).  Only the weight stream of the mode in use is packed and
// uploaded; another mode's is built on its first selection.
struct ModeDesc {
    int id;
    size_t (*ws_floats)(size_t n);          // scratch of a launch of n proposal slots (the batched FC tail and what the mode adds)
    int (*launch)(const RegressArgs &a, int n, hipStream_t stream);
};
// the direct mode only parks the pooled features and the next level's proposals; the Winograd mode also a chunk's transformed conv2 input
static const ModeDesc MODES[P2P_REGRESS_NMODES] = {
    {P2P_REGRESS_F32, [](size_t) -> size_t { return 0; }, launch_regress_f32},
    {P2P_REGRESS_FP16X2, regress_ws_base_floats, launch_regress_h2},
    {P2P_REGRESS_FP16X2W, regress_ws_floats, launch_regress_wino},
    {P2P_REGRESS_FP16, regress_ws_floats_fp16, fp16x1::launch_regress_wino},
};
// row of MODES (= slot of the handle's stream[] and view[]), -1 for an unknown mode
static int mode_index(int mode) {
    for (int m = 0; m < P2P_REGRESS_NMODES; ++m)
        if (MODES[m].id == mode) return m;
    return -1;
}

// pack + upload the convolution weights in the stream order of `mode`'s kernels, complete the mode's view (once per handle and mode)
static int ensure_mode(p2p_regressor *r, int mode) {
    const int m = mode_index(mode);
    DeviceBlob &blob = r->stream[m];
    if (blob.uploaded()) return P2P_OK;
    // the parts of the mode's blob: the RegDev pointer each becomes, at which float it starts
    struct Part { const float *RegDev::*field; size_t off; };
    std::vector<Part> parts;
    DeviceBlob b;
    auto take = [&](const float *RegDev::*field, size_t floats) {
        parts.push_back({field, b.take<float>(floats)});
        return parts.back().off;
    };
    const float *c1 = r->conv1_w.data(), *c2 = r->conv2_w.data(), *bn1s = r->bn1s_host.data(), *bn2s = r->bn2s_host.data();
    std::vector<int> t1(512), t2(512);
    const char *what;
    // fp16 modes: conv1 accumulates 2^12 (activations) x 2^t1[n] (weights) x the true sum, conv2 2^t2[n] x (the per-proposal scale
    // of H, undone in the kernel) x the true sum: exact powers of two folded into the BatchNorm scales
    if (mode == P2P_REGRESS_F32) {
        const size_t o1 = take(&RegDev::wp1, WP1_FLOATS), o2 = take(&RegDev::wp2, WP2_FLOATS);
        pack_f32_weights(c1, c2, b.at<float>(o1), b.at<float>(o2));
        what = "the f32 weight streams";
    } else if (mode == P2P_REGRESS_FP16X2) {
        const size_t o1 = take(&RegDev::wh1, WH1_FLOATS), o2 = take(&RegDev::wh2, WH2_FLOATS);
        const size_t ob1 = take(&RegDev::bn1s_h, 512), ob2 = take(&RegDev::bn2s_h, 512);
        pack_h2_weights(c1, c2, b.at<float>(o1), b.at<float>(o2), t1.data(), t2.data());
        fold_exponent(bn1s, t1.data(), 12, b.at<float>(ob1));
        fold_exponent(bn2s, t2.data(), 0, b.at<float>(ob2));
        what = "the fp16x2 weight streams";
    } else if (mode == P2P_REGRESS_FP16) {
        // the structure of P2P_REGRESS_FP16X2W with one fp16 plane per operand: half the bytes of both streams
        const size_t o2 = take(&RegDev::ww2, WW2_FLOATS_FP16), ob2 = take(&RegDev::bn2s_w, 512);
        const size_t o1 = take(&RegDev::wh1, WH1_FLOATS_FP16), ob1 = take(&RegDev::bn1s_h, 512);
        fp16x1::pack_wino_weights(c2, b.at<float>(o2), t2.data());
        fp16x1::pack_h2_weights(c1, nullptr, b.at<float>(o1), nullptr, t1.data(), nullptr);
        fold_exponent(bn1s, t1.data(), 12, b.at<float>(ob1));
        fold_exponent(bn2s, t2.data(), 0, b.at<float>(ob2));
        what = "the single-plane Winograd filter blocks and conv1's stream";
    } else {
        // conv2 as Winograd filter blocks + conv1's fp16x2 stream (the same stream the direct mode runs, packed here on its own:
        // the direct mode's conv2 stream -- 9.6 MB per regressor -- is neither packed nor uploaded for this mode)
        const size_t o2 = take(&RegDev::ww2, WW2_FLOATS), ob2 = take(&RegDev::bn2s_w, 512);
        const size_t o1 = take(&RegDev::wh1, WH1_FLOATS), ob1 = take(&RegDev::bn1s_h, 512);
        pack_wino_weights(c2, b.at<float>(o2), t2.data());
        pack_h2_weights(c1, nullptr, b.at<float>(o1), nullptr, t1.data(), nullptr);
        fold_exponent(bn1s, t1.data(), 12, b.at<float>(ob1));
        fold_exponent(bn2s, t2.data(), 0, b.at<float>(ob2));
        what = "the Winograd filter blocks and conv1's stream";
    }
    const int st = b.upload(what);
    if (st != P2P_OK) return st;
    blob = std::move(b);
    r->view[m] = r->common;
    for (const Part &q : parts) r->view[m].*q.field = blob.dev<float>(q.off);
    return P2P_OK;
}

extern "C" int p2p_regressor_set_mode(p2p_regressor *reg, int mode) {
    P2P_REQUIRE(reg, P2P_EINVAL, "p2p_regressor_set_mode: null handle");
    const bool generic_id = mode == P2P_REGRESS_GENERIC || mode == P2P_REGRESS_GENERIC_FP16X2;
    if (reg->gen) {
        P2P_REQUIRE(generic_id || mode_index(mode) >= 0, P2P_EINVAL, "p2p_regressor_set_mode: unknown mode %d", mode);
        P2P_REQUIRE(generic_id, P2P_EUNSUPPORTED,
                    "p2p_regressor_set_mode: a generic regressor (p2p_regressor_create_config) runs P2P_REGRESS_GENERIC or "
                    "P2P_REGRESS_GENERIC_FP16X2, not the tuned mode %d", mode);
        if (mode == P2P_REGRESS_GENERIC_FP16X2) {       // the planes are allocated on the HANDLE's device
            int cur = 0;
            P2P_HIP_CHECK(hipGetDevice(&cur));
            if (cur != reg->device) P2P_HIP_CHECK(hipSetDevice(reg->device));
            const int st = regressor_generic_ensure_h2(reg->gen);
            if (cur != reg->device) P2P_HIP_CHECK(hipSetDevice(cur));
            if (st != P2P_OK) return st;
        }
        reg->mode = reg->gen->mode = mode;
        return P2P_OK;
    }
    P2P_REQUIRE(!generic_id, P2P_EUNSUPPORTED,
                "p2p_regressor_set_mode: mode %d needs a handle made by p2p_regressor_create_config", mode);
    P2P_REQUIRE(mode_index(mode) >= 0, P2P_EINVAL, "p2p_regressor_set_mode: unknown mode %d", mode);
    // the weight stream of a mode is allocated on the HANDLE's device, whatever the caller's current device is
    int cur = 0;
    P2P_HIP_CHECK(hipGetDevice(&cur));
    if (cur != reg->device) P2P_HIP_CHECK(hipSetDevice(reg->device));
    const int st = ensure_mode(reg, mode);
    if (cur != reg->device) P2P_HIP_CHECK(hipSetDevice(cur));
    if (st != P2P_OK) return st;
    reg->mode = mode;
    return P2P_OK;
}

extern "C" int p2p_regressor_get_mode(const p2p_regressor *reg) { return reg ? reg->mode : P2P_EINVAL; }

extern "C" int p2p_regressor_create(const p2p_regressor_params *p, p2p_regressor **out) {
    P2P_REQUIRE(p && out, P2P_EINVAL, "p2p_regressor_create: null argument");
    const float *const need[] = {p->conv1_w, p->conv2_w, p->fc1_w, p->fc1_b, p->fc2_w, p->fc2_b, p->fc3_w, p->fc3_b,
                                 p->bn1.weight, p->bn1.bias, p->bn1.running_mean, p->bn1.running_var,
                                 p->bn2.weight, p->bn2.bias, p->bn2.running_mean, p->bn2.running_var,
                                 p->bnf1.weight, p->bnf1.bias, p->bnf1.running_mean, p->bnf1.running_var,
                                 p->bnf2.weight, p->bnf2.bias, p->bnf2.running_mean, p->bnf2.running_var};
    for (const float *q : need) P2P_REQUIRE(q, P2P_EINVAL, "p2p_regressor_create: null weight pointer");

    // everything but the convolution weights (which are packed per arithmetic mode, ensure_mode): one blob
    p2p_regressor *r = new p2p_regressor();      // value-initialised: no stream, every view empty
    DeviceBlob &b = r->dev;
    auto take = [&](size_t n) { return b.take<float>(n); };
    const size_t o_bn1s = take(512), o_bn1b = take(512), o_bn2s = take(512), o_bn2b = take(512);
    const size_t o_fc1t = take(512 * 512), o_fc1b = take(512), o_bnf1s = take(512), o_bnf1b = take(512);
    const size_t o_fc2t = take(256 * 512), o_fc2b = take(256), o_bnf2s = take(256), o_bnf2b = take(256);
    const size_t o_fc3 = take(5 * 256), o_fc3b = take(8);
    const size_t o_fc1p = take(512 * 512), o_fc2p = take(256 * 512);
    float *h = b.at<float>(0);
    fold_bn(p->bn1, 512, &h[o_bn1s], &h[o_bn1b]);
    fold_bn(p->bn2, 512, &h[o_bn2s], &h[o_bn2b]);
    fold_bn(p->bnf1, 512, &h[o_bnf1s], &h[o_bnf1b]);
    fold_bn(p->bnf2, 256, &h[o_bnf2s], &h[o_bnf2b]);
    // fc weights as [k/4][out][4] so that a wave reads 1 KiB contiguous per step (per-proposal tail of the f32 kernel)
    for (int o = 0; o < 512; ++o)
        for (int k = 0; k < 512; ++k) h[o_fc1t + ((size_t)(k / 4) * 512 + o) * 4 + (k & 3)] = p->fc1_w[(size_t)o * 512 + k];
    for (int o = 0; o < 256; ++o)
        for (int k = 0; k < 512; ++k) h[o_fc2t + ((size_t)(k / 4) * 256 + o) * 4 + (k & 3)] = p->fc2_w[(size_t)o * 512 + k];
    pack_fc_mfma(p->fc1_w, 512, 512, &h[o_fc1p]);      // the same two layers as MFMA fragments (batched tail of the fp16x2 kernel)
    pack_fc_mfma(p->fc2_w, 256, 512, &h[o_fc2p]);
    for (int i = 0; i < 512; ++i) h[o_fc1b + i] = p->fc1_b[i];
    for (int i = 0; i < 256; ++i) h[o_fc2b + i] = p->fc2_b[i];
    for (int i = 0; i < 5 * 256; ++i) h[o_fc3 + i] = p->fc3_w[i];
    for (int i = 0; i < 5; ++i) h[o_fc3b + i] = p->fc3_b[i];
    r->conv1_w.assign(p->conv1_w, p->conv1_w + (size_t)512 * 518 * 9);      // host copies: another mode's stream is packed on demand
    r->conv2_w.assign(p->conv2_w, p->conv2_w + (size_t)512 * 512 * 9);
    r->bn1s_host.assign(&h[o_bn1s], &h[o_bn1s] + 512);
    r->bn2s_host.assign(&h[o_bn2s], &h[o_bn2s] + 512);

    int st = b.upload("the regressor's BatchNorm / FC parameters");
    if (st == P2P_OK) {
        (void)hipGetDevice(&r->device);
        RegDev &c = r->common;
        const float *dev = b.dev<float>();
        c.bn1s = dev + o_bn1s; c.bn1b = dev + o_bn1b; c.bn2s = dev + o_bn2s; c.bn2b = dev + o_bn2b;
        c.fc1t = dev + o_fc1t; c.fc1b = dev + o_fc1b; c.bnf1s = dev + o_bnf1s; c.bnf1b = dev + o_bnf1b;
        c.fc2t = dev + o_fc2t; c.fc2b = dev + o_fc2b; c.bnf2s = dev + o_bnf2s; c.bnf2b = dev + o_bnf2b;
        c.fc3 = dev + o_fc3; c.fc3b = dev + o_fc3b;
        c.fc1p = dev + o_fc1p; c.fc2p = dev + o_fc2p;
        r->mode = P2P_REGRESS_DEFAULT;
        st = ensure_mode(r, r->mode);
    }
    if (st != P2P_OK) {
        delete r;
        return st;
    }
    *out = r;
    return P2P_OK;
}

extern "C" int p2p_regressor_create_config(const p2p_regressor_config *config, const p2p_regressor_tensors *tensors,
                                           p2p_regressor **out) {
    GenReg *g = nullptr;
    const int st = regressor_generic_create(config, tensors, &g);
    if (st != P2P_OK) return st;
    p2p_regressor *r = new p2p_regressor();      // value-initialised: no tuned stream or view
    (void)hipGetDevice(&r->device);
    r->mode = P2P_REGRESS_GENERIC;
    r->gen = g;
    *out = r;
    return P2P_OK;
}

extern "C" void p2p_regressor_destroy(p2p_regressor *reg) { delete reg; }

// counts: per item, the number of slots in the concatenated arrays (host memory); dev_counts (optional, device
// memory, indexed like counts): how many of those slots hold a proposal -- the remaining work-groups exit at once.
static int regress_batch_impl(const p2p_regressor *reg1, const p2p_regressor *reg2, int nitems,
                              const p2p_pyramid *im1, const p2p_pyramid *im2, const int *counts, const int *dev_counts,
                              const void *proposals, int is_float,
                              float *matches1, float *probs1, float *raw1,
                              float *matches2, float *probs2, float *raw2, void *workspace, size_t workspace_bytes,
                              p2p_stream_t stream) {
    P2P_REQUIRE(reg1 && im1 && im2 && counts, P2P_EINVAL, "p2p_regress: null argument");
    P2P_REQUIRE(nitems >= 0, P2P_EINVAL, "p2p_regress: negative item count");
    long long total = 0;
    for (int i = 0; i < nitems; ++i) {
        P2P_REQUIRE(counts[i] >= 0, P2P_EINVAL, "p2p_regress: negative proposal count");
        total += counts[i];
    }
    if (total == 0) return P2P_OK;
    P2P_REQUIRE(total < (1ll << 31), P2P_EINVAL, "p2p_regress: too many proposals");
    P2P_REQUIRE(proposals, P2P_EINVAL, "p2p_regress: null proposals");
    P2P_REQUIRE(reg2 ? (matches2 && probs2) : (matches1 && probs1), P2P_EINVAL, "p2p_regress: missing output buffers");
    P2P_REQUIRE(!reg2 || !reg2->gen == !reg1->gen, P2P_EINVAL, "p2p_regress: a generic and a tuned regressor cannot be chained");
    P2P_REQUIRE(!reg2 || !reg1->gen || memcmp(&reg1->gen->cfg, &reg2->gen->cfg, sizeof(p2p_regressor_config)) == 0, P2P_EINVAL,
                "p2p_regress: the two generic regressors have different configurations");
    P2P_REQUIRE(!reg2 || reg2->mode == reg1->mode, P2P_EINVAL, "p2p_regress: the two regressors use different arithmetic modes (%d and %d)",
                reg1->mode, reg2->mode);
    for (int i = 0; i < nitems; ++i) {
        const p2p_pyramid *im[2] = {im1 + i, im2 + i};
        for (int s = 0; s < 2; ++s) {
            P2P_REQUIRE(im[s]->height >= 8 && im[s]->width >= 8 && im[s]->height < 32768 && im[s]->width < 32768,
                        P2P_EINVAL, "p2p_regress: item %d image %d size %dx%d must be within [8, 32767]", i, s + 1,
                        im[s]->height, im[s]->width);
            for (int j = 0; j < 4; ++j) P2P_REQUIRE(im[s]->level[j], P2P_EINVAL, "p2p_regress: null pyramid level");
        }
    }
    const int m = mode_index(reg1->mode);
    int most = 0;      // proposal slots of the largest launch
    for (int i0 = 0; i0 < nitems; i0 += MAXB) {
        int n = 0;
        for (int b = i0; b < nitems && b < i0 + MAXB; ++b) n += counts[b];
        most = std::max(most, n);
    }
    // a generic regressor needs one unit of 8 proposals at least and cuts its chunk to what it is given
    const size_t need = reg1->gen ? gen_per_prop(*reg1->gen) * GEN_UNIT * sizeof(float) : MODES[m].ws_floats((size_t)most) * sizeof(float);
    if (need) {
        P2P_REQUIRE(workspace && ((uintptr_t)workspace & 127) == 0, P2P_EINVAL,
                    "p2p_regress: a 128-byte aligned workspace of %zu bytes (p2p_regress_workspace_bytes_mode) is needed", need);
        // too small: P2P_ENOMEM like every other workspace check of the library (a caller may grow the buffer and retry)
        P2P_REQUIRE(workspace_bytes >= need, P2P_ENOMEM,
                    "p2p_regress: workspace of %zu bytes (p2p_regress_workspace_bytes_mode) needed, got %zu", need, workspace_bytes);
    }
    // launches of at most MAXB items; outputs/proposals are indexed by the global proposal number
    int first_prop = 0;
    for (int i0 = 0; i0 < nitems; i0 += MAXB) {
        const int nb = (nitems - i0 < MAXB) ? nitems - i0 : MAXB;
        RegressArgs a;
        int n = 0;
        for (int b = 0; b < nb; ++b) {
            const p2p_pyramid *im[2] = {im1 + i0 + b, im2 + i0 + b};
            for (int s = 0; s < 2; ++s) {
                for (int j = 0; j < 4; ++j) a.item[b].pyr[s][j] = im[s]->level[j];
                a.item[b].H[s] = im[s]->height;
                a.item[b].W[s] = im[s]->width;
            }
            a.start[b] = n;
            n += counts[i0 + b];
        }
        for (int b = nb; b <= MAXB; ++b) a.start[b] = n;
        for (int b = nb; b < MAXB; ++b) a.item[b] = a.item[0];
        a.nitems = nb;
        a.dev_counts = dev_counts ? dev_counts + i0 : nullptr;
        a.is_float = is_float; a.n = n; a.nlevels = reg2 ? 2 : 1;
        a.proposals = is_float ? (const void *)((const float *)proposals + (size_t)first_prop * 4)
                               : (const void *)((const long long *)proposals + (size_t)first_prop * 4);
        a.reg[0] = reg1->gen ? RegDev{} : reg1->view[m];
        a.reg[1] = reg2 && !reg2->gen ? reg2->view[m] : a.reg[0];
        auto adv = [&](float *p, int cols) { return p ? p + (size_t)first_prop * cols : nullptr; };
        a.matches[0] = adv(matches1, 4); a.probs[0] = adv(probs1, 1); a.raw[0] = adv(raw1, 5);
        a.matches[1] = adv(matches2, 4); a.probs[1] = adv(probs2, 1); a.raw[1] = adv(raw2, 5);
        a.ws = (float *)workspace;      // launches of one call are ordered on the stream: they may share the scratch
        if (n > 0) {
            a.wU = nullptr; a.hinv = nullptr; a.lvl0 = 0; a.p0 = 0; a.p1 = n; a.mblocks = 0;
            const int st = reg1->gen ? launch_regress_generic(*reg1->gen, reg2 ? reg2->gen : nullptr, a, n, workspace_bytes,
                                                              (hipStream_t)stream)
                                     : MODES[m].launch(a, n, (hipStream_t)stream);
            if (st != P2P_OK) return st;
        }
        first_prop += n;
    }
    return P2P_OK;
}

extern "C" int p2p_regress_batch(const p2p_regressor *reg1, const p2p_regressor *reg2, int nitems,
                                 const p2p_pyramid *im1, const p2p_pyramid *im2, const int *counts,
                                 const void *proposals, int is_float,
                                 float *matches1, float *probs1, float *raw1,
                                 float *matches2, float *probs2, float *raw2, void *workspace, size_t workspace_bytes,
                                 p2p_stream_t stream) {
    return regress_batch_impl(reg1, reg2, nitems, im1, im2, counts, nullptr, proposals, is_float, matches1, probs1, raw1,
                              matches2, probs2, raw2, workspace, workspace_bytes, stream);
}

extern "C" size_t p2p_regress_workspace_bytes(int n) {
    return n > 0 ? regress_ws_floats((size_t)n) * sizeof(float) : 0;
}

extern "C" size_t p2p_regress_workspace_bytes_mode(int n, int mode) {
    if (n <= 0) return 0;
    const int m = mode_index(mode);      // a mode the library does not know gets the direct mode's answer, as it always has
    return (m >= 0 ? MODES[m].ws_floats : regress_ws_base_floats)((size_t)n) * sizeof(float);
}

extern "C" size_t p2p_regress_workspace_bytes_for(const p2p_regressor *reg, int n) {
    if (!reg || n <= 0) return 0;
    if (!reg->gen) return p2p_regress_workspace_bytes_mode(n, reg->mode);
    const size_t units = ((size_t)std::min(n, GEN_CAP) + GEN_UNIT - 1) / GEN_UNIT;
    return units * GEN_UNIT * gen_per_prop(*reg->gen) * sizeof(float);      // by the handle's mode
}

extern "C" int p2p_regress_batch_dev(const p2p_regressor *reg1, const p2p_regressor *reg2, int nitems,
                                     const p2p_pyramid *im1, const p2p_pyramid *im2, const int *dev_counts, int stride,
                                     const void *proposals, int is_float,
                                     float *matches1, float *probs1, float *raw1,
                                     float *matches2, float *probs2, float *raw2, void *workspace, size_t workspace_bytes,
                                     p2p_stream_t stream) {
    P2P_REQUIRE(dev_counts && stride >= 1 && nitems >= 0 && nitems <= 4096, P2P_EINVAL, "p2p_regress_batch_dev: bad argument");
    std::vector<int> cap(nitems, stride);
    return regress_batch_impl(reg1, reg2, nitems, im1, im2, cap.data(), dev_counts, proposals, is_float, matches1, probs1,
                              raw1, matches2, probs2, raw2, workspace, workspace_bytes, stream);
}

extern "C" int p2p_regress(const p2p_regressor *reg1, const p2p_regressor *reg2,
                           const p2p_pyramid *im1, const p2p_pyramid *im2,
                           const void *proposals, int is_float, int n,
                           float *matches1, float *probs1, float *raw1,
                           float *matches2, float *probs2, float *raw2, void *workspace, size_t workspace_bytes,
                           p2p_stream_t stream) {
    P2P_REQUIRE(n >= 0, P2P_EINVAL, "p2p_regress: negative proposal count");
    return p2p_regress_batch(reg1, reg2, 1, im1, im2, &n, proposals, is_float, matches1, probs1, raw1, matches2, probs2,
                             raw2, workspace, workspace_bytes, stream);
}
