// The matching operators as entry points of their own (include/p2p_hip.h, "matching operators"): argument checks -- all before the
// device is touched -- and the calls of the launchers (operators.hip, coarse.hip, consensus_generic.hip; declared in
// coarse_common.h).  No kernel lives here.  Compiled as part of api.hip, not as a unit of its own.
#include "coarse_common.h"

using namespace p2p;

static bool op_batch_ok(int batch) { return batch >= 1 && batch <= 65535; }
static long long op_area(int h, int w) { return (long long)h * w; }

extern "C" int p2p_correlation_batch(const float *featA, const float *featB, int batch, int channels, int hA, int wA, int hB, int wB,
                                     float *out, p2p_stream_t stream) {
    P2P_REQUIRE(featA && featB && out, P2P_EINVAL, "p2p_correlation: null argument");
    P2P_REQUIRE(op_batch_ok(batch), P2P_EINVAL, "p2p_correlation: batch %d out of range", batch);
    P2P_REQUIRE(channels > 0 && hA > 0 && wA > 0 && hB > 0 && wB > 0, P2P_EINVAL, "p2p_correlation: channels and sides must be positive");
    const long long nA = op_area(hA, wA), nB = op_area(hB, wB);
    // a work-group owns 64 A positions (grid y), positions are 32-bit
    P2P_REQUIRE(nA <= 65535ll * 64 && nB < (1ll << 31) - 64, P2P_EUNSUPPORTED, "p2p_correlation: %lld x %lld positions in one launch", nA, nB);
    launch_correlation(CorrelationArgs{featA, featB, out, channels, (int)nA, (int)nB, (size_t)channels * nA, (size_t)channels * nB,
                                       (size_t)nA * nB}, batch, (hipStream_t)stream);
    return check_launch("correlation_kernel");
}

extern "C" int p2p_maxpool4d_batch(const float *x, int batch, int h1, int w1, int h2, int w2, int k, float *pooled_out,
                                   uint8_t *delta_out, p2p_stream_t stream) {
    P2P_REQUIRE(x && pooled_out, P2P_EINVAL, "p2p_maxpool4d: null argument");
    P2P_REQUIRE(op_batch_ok(batch), P2P_EINVAL, "p2p_maxpool4d: batch %d out of range", batch);
    P2P_REQUIRE(h1 > 0 && w1 > 0 && h2 > 0 && w2 > 0 && k > 0, P2P_EINVAL, "p2p_maxpool4d: sides and k must be positive");
    P2P_REQUIRE(k <= 4, P2P_EUNSUPPORTED, "p2p_maxpool4d: k %d: the k^4 codes must fit a byte (1 to 4)", k);
    P2P_REQUIRE(h1 % k == 0 && w1 % k == 0 && h2 % k == 0 && w2 % k == 0, P2P_EINVAL, "p2p_maxpool4d: sides must be multiples of k = %d", k);
    const size_t cells = (size_t)(h1 / k) * (w1 / k) * (h2 / k) * (w2 / k);
    P2P_REQUIRE(cells < ((size_t)1 << 38), P2P_EUNSUPPORTED, "p2p_maxpool4d: %zu pooled cells in one launch", cells);
    launch_maxpool4d(MaxPool4dArgs{x, pooled_out, delta_out, k, w1 / k, h2 / k, w2 / k, cells}, batch, (hipStream_t)stream);
    return check_launch("maxpool4d_kernel");
}

// per item: the row keys, then the column keys, each padded to four words (16-byte loads of the apply kernel)
static size_t mm_keys_per_item(long long nA, long long nB) { return (size_t)(((nA + 3) & ~3ll) + ((nB + 3) & ~3ll)); }

extern "C" size_t p2p_mutual_matching_workspace_bytes(int batch, int hA, int wA, int hB, int wB) {
    if (!op_batch_ok(batch) || hA <= 0 || wA <= 0 || hB <= 0 || wB <= 0) return 0;
    return (size_t)batch * mm_keys_per_item(op_area(hA, wA), op_area(hB, wB)) * sizeof(int);
}

extern "C" int p2p_mutual_matching_batch(const float *x, int batch, int hA, int wA, int hB, int wB, float *y_out, void *workspace,
                                         size_t workspace_bytes, p2p_stream_t stream) {
    P2P_REQUIRE(x && y_out, P2P_EINVAL, "p2p_mutual_matching: null argument");
    P2P_REQUIRE(op_batch_ok(batch), P2P_EINVAL, "p2p_mutual_matching: batch %d out of range", batch);
    P2P_REQUIRE(hA > 0 && wA > 0 && hB > 0 && wB > 0, P2P_EINVAL, "p2p_mutual_matching: sides must be positive");
    const long long nA = op_area(hA, wA), nB = op_area(hB, wB);
    // mm_apply_kernel indexes an item's cells with 32-bit values
    P2P_REQUIRE(nA < (1ll << 30) && nB < (1ll << 30) && nA * nB < (1ll << 31), P2P_EUNSUPPORTED,
                "p2p_mutual_matching: %lld x %lld cells per item (fewer than 2^31 are implemented)", nA, nB);
    const size_t need = p2p_mutual_matching_workspace_bytes(batch, hA, wA, hB, wB);
    P2P_REQUIRE(workspace && workspace_bytes >= need, P2P_ENOMEM, "p2p_mutual_matching: workspace of %zu bytes needed", need);
    P2P_REQUIRE(((uintptr_t)workspace & 3) == 0, P2P_EINVAL, "p2p_mutual_matching: the workspace must be 4-byte aligned");
    launch_mutual_matching(x, (int)nA, (int)nB, y_out, (int *)workspace, mm_keys_per_item(nA, nB), batch, (hipStream_t)stream);
    return check_launch("mutual matching kernels");
}

extern "C" int p2p_conv4d_create(const float *weight, const float *bias, int c_in, int c_out, int kernel_size, p2p_conv4d **out) {
    P2P_REQUIRE(weight && out, P2P_EINVAL, "p2p_conv4d_create: null argument");
    P2P_REQUIRE(c_in > 0 && c_out > 0 && kernel_size > 0, P2P_EINVAL, "p2p_conv4d_create: channels %d -> %d, kernel_size %d must be positive",
                c_in, c_out, kernel_size);
    P2P_REQUIRE(kernel_size == 3 || kernel_size == 5, P2P_EUNSUPPORTED, "p2p_conv4d_create: kernel_size %d: kernel sizes 3 and 5 are implemented",
                kernel_size);
    P2P_REQUIRE(c_in <= 16 && c_out <= 16, P2P_EUNSUPPORTED, "p2p_conv4d_create: channels %d -> %d: at most 16 are implemented", c_in, c_out);
    Conv4dLayer *layer = nullptr;
    const int st = conv4d_create(weight, bias, c_in, c_out, kernel_size, &layer);
    if (st != P2P_OK) return st;
    *out = new p2p_conv4d{layer};
    return P2P_OK;
}

extern "C" void p2p_conv4d_destroy(p2p_conv4d *conv) { delete conv; }

extern "C" int p2p_conv4d_forward_batch(const p2p_conv4d *conv, const float *x, int batch, int h1, int w1, int h2, int w2, float *y_out,
                                        p2p_stream_t stream) {
    P2P_REQUIRE(conv && x && y_out, P2P_EINVAL, "p2p_conv4d_forward: null argument");
    P2P_REQUIRE(op_batch_ok(batch), P2P_EINVAL, "p2p_conv4d_forward: batch %d out of range", batch);
    P2P_REQUIRE(h1 > 0 && w1 > 0 && h2 > 0 && w2 > 0, P2P_EINVAL, "p2p_conv4d_forward: sides must be positive");
    P2P_REQUIRE(x != y_out, P2P_EINVAL, "p2p_conv4d_forward: the layer cannot run in place");
    return launch_conv4d(*conv->layer, x, y_out, batch, h1, w1, h2, w2, (hipStream_t)stream);
}

extern "C" int p2p_l2_normalize(const float *x, size_t outer, int channels, size_t inner, float *y, p2p_stream_t stream) {
    P2P_REQUIRE(x && y, P2P_EINVAL, "p2p_l2_normalize: null argument");
    P2P_REQUIRE(outer > 0 && channels > 0 && inner > 0, P2P_EINVAL, "p2p_l2_normalize: sizes must be positive");
    P2P_REQUIRE(outer < ((size_t)1 << 38) && inner < ((size_t)1 << 38) && outer * inner < ((size_t)1 << 38), P2P_EUNSUPPORTED,
                "p2p_l2_normalize: %zu x %zu positions in one launch", outer, inner);
    launch_l2_normalize(x, outer, channels, inner, y, (hipStream_t)stream);
    return check_launch("l2_normalize_kernel");
}
