// TEST INFRASTRUCTURE: a stand-alone program over patch2pix_amd/csrc/host_pack.h, compiled against the HIP stand-in of this
// directory with -fsanitize=address,undefined (tests/test_host_pack.py).  It launches no kernel: it lays out, fills, uploads,
// moves and releases blobs, refuses an allocation, and compares the shared arithmetic with naive restatements written here.
// Exit status 0 and "host_pack_test: ok" on success; the sanitizers report leaks and undefined behaviour on their own.
#include "../../patch2pix_amd/csrc/host_pack.h"

#include <cstdarg>
#include <cstring>
#include <limits>
#include <string>

static char g_error[512];
namespace p2p {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}
}  // namespace p2p
using namespace p2p;

static int g_failed = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

static uint16_t half_bits(float v) { const _Float16 h = (_Float16)v; uint16_t u; memcpy(&u, &h, 2); return u; }
static float half_value(uint16_t u) { _Float16 h; memcpy(&h, &u, 2); return (float)h; }

static void test_layout_and_upload() {
    DeviceBlob b;
    const size_t counts[] = {1, 64, 65, 512, 5, 1000};
    size_t off[6], end = 0;
    for (int i = 0; i < 6; ++i) {
        off[i] = b.take<float>(counts[i]);
        CHECK(off[i] % 64 == 0);                 // a multiple of 64 elements
        CHECK(off[i] >= end);                    // no overlap with the part before
        end = off[i] + counts[i];
    }
    CHECK(b.bytes() % 256 == 0 && b.bytes() >= end * sizeof(float));
    CHECK(!b.uploaded());
    for (int i = 0; i < 6; ++i)
        for (size_t q = 0; q < counts[i]; ++q) b.at<float>(off[i])[q] = (float)(1000 * (i + 1) + q);
    const std::vector<unsigned char> staged(b.at<unsigned char>(0), b.at<unsigned char>(0) + b.bytes());
    CHECK(b.upload("test blob") == P2P_OK && b.uploaded());
    CHECK(memcmp(b.dev<unsigned char>(), staged.data(), staged.size()) == 0);      // (the stand-in's device memory is host memory)
    for (int i = 0; i < 6; ++i) {
        const float *part = b.dev<float>(off[i]);
        const size_t next = i < 5 ? off[i + 1] : b.bytes() / sizeof(float);
        for (size_t q = 0; q < counts[i]; ++q) CHECK(part[q] == (float)(1000 * (i + 1) + q));
        for (size_t q = counts[i]; q < next - off[i]; ++q) CHECK(part[q] == 0.f);  // padding
    }
    // bytes, then floats, as the convolution blobs: the float parts start where the bytes end
    DeviceBlob m;
    const size_t ow = m.take<unsigned char>(2048), os = m.take<float>(64), oh = m.take<float>(64);
    CHECK(ow == 0 && os == 512 && oh == 576 && m.bytes() == 2048 + 2 * 256);
    m.at<unsigned char>(ow)[2047] = 7;
    m.at<float>(os)[0] = 1.5f;
    CHECK(m.upload("mixed blob") == P2P_OK);
    CHECK(m.dev<unsigned char>(ow)[2047] == 7 && m.dev<float>(os)[0] == 1.5f && m.dev<float>(oh)[63] == 0.f);

    // move, release, release again; a blob that was never uploaded
    const unsigned char *before = b.dev<unsigned char>();
    DeviceBlob c(std::move(b));
    CHECK(!b.uploaded() && c.uploaded() && c.dev<unsigned char>() == before);
    DeviceBlob d;
    d = std::move(c);
    CHECK(!c.uploaded() && d.uploaded() && d.dev<unsigned char>() == before);
    d.release();
    CHECK(!d.uploaded());
    d.release();
    b.release();
    DeviceBlob never;
    never.take<float>(100);
    never.at<float>(0)[99] = 1.f;
    never.release();
}

static void test_refused_allocation() {
    DeviceBlob b;
    b.at<float>(b.take<float>(700))[699] = 3.f;
    g_error[0] = 0;
    hipemu::refuse_allocs = 1;
    CHECK(b.upload("refused blob") == P2P_ENOMEM);
    CHECK(!b.uploaded() && hipemu::refuse_allocs == 0);
    CHECK(strlen(g_error) > 0 && strstr(g_error, "refused blob") && strstr(g_error, "2816 bytes"));
    b.release();
}

// the values the old copies could have disagreed on, and a few dozen ordinary ones
static std::vector<float> interesting() {
    std::vector<float> v = {0.f, -0.f, 2048.f, -2048.f, 4096.f, 4095.75f, 1.f, 0.5f, 1e-3f, -7.25f, 65504.f, 70000.f, 1e-8f, 1e-40f,
                            std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                            std::numeric_limits<float>::quiet_NaN(), 1.f + 0x1p-20f /* low plane 2^-20: an fp16 subnormal */,
                            3.f - 0x1p-17f};
    unsigned s = 12345;
    for (int i = 0; i < 40; ++i) {
        s = s * 1664525u + 1013904223u;
        v.push_back(std::ldexp((float)((int)(s >> 8) - (1 << 23)) / (float)(1 << 23), (int)(s & 31) - 16));
    }
    return v;
}

static void test_arithmetic() {
    const std::vector<float> vals = interesting();
    for (float v : vals) {
        uint16_t hi = 1, lo = 1;
        split_fp16_planes(v, &hi, &lo);
        const uint16_t want_hi = half_bits(v), want_lo = half_bits(v - half_value(want_hi));
        CHECK(hi == want_hi && lo == want_lo);
        // the exponent: by search instead of frexp
        for (int target : {12, 13}) {
            int want = 0;
            const double a = std::fabs((double)v);
            if (a > 0.0 && std::isfinite(a)) {
                want = -400;
                while (!(std::ldexp(a, want) >= std::ldexp(1.0, target - 1))) ++want;
                CHECK(std::ldexp(a, want) < std::ldexp(1.0, target));
            }
            CHECK(pow2_exponent_to(std::fabs(v), target) == want);
            CHECK(pow2_exponent_to(std::fabs((double)v), target) == want);
        }
    }
    CHECK(pow2_exponent_to(2048.f, 12) == 0 && pow2_exponent_to(4096.f, 12) == -1 && pow2_exponent_to(0.f, 12) == 0);
    CHECK(pow2_exponent_to(std::numeric_limits<double>::infinity(), 12) == 0);
    {   // a low plane that is an fp16 subnormal survives
        uint16_t hi, lo;
        split_fp16_planes(1.f + 0x1p-20f, &hi, &lo);
        CHECK(half_value(hi) == 1.f && half_value(lo) == 0x1p-20f && (lo & 0x7c00) == 0 && lo != 0);
    }

    // fold_bn on 48 channels, a zero weight, a zero variance and a huge variance among them
    const int n = 48;
    std::vector<float> w(n), bias(n), mean(n), var(n), scale(n), shift(n);
    for (int i = 0; i < n; ++i) {
        w[i] = vals[(i + 5) % vals.size()]; bias[i] = 0.25f * i - 3.f; mean[i] = 1.f / (i + 1) - 0.5f; var[i] = 0.01f * i * i;
    }
    w[3] = 0.f; var[7] = 1e30f; w[11] = 2048.f;
    for (float &x : w) if (!std::isfinite(x)) x = 1.f;
    const p2p_bn_params bn{w.data(), bias.data(), mean.data(), var.data()};
    fold_bn(bn, n, scale.data(), shift.data());
    for (int i = 0; i < n; ++i) {
        const float inv = 1.0f / std::sqrt(var[i] + 1e-5f), s = w[i] * inv;
        CHECK(scale[i] == s && shift[i] == bias[i] - mean[i] * s);
    }

    // pack_fc_mfma against its definition, entry by entry
    const int shapes[][2] = {{32, 16}, {32, 48}, {16, 512}};
    for (const auto &sh : shapes) {
        const int N = sh[0], K = sh[1];
        std::vector<float> W((size_t)N * K), out((size_t)N * K, -1.f);
        for (size_t i = 0; i < W.size(); ++i) W[i] = (float)i + 0.5f;
        pack_fc_mfma(W.data(), N, K, out.data());
        std::vector<int> seen(W.size(), 0);
        for (int row = 0; row < N; ++row)
            for (int col = 0; col < K; ++col) {
                const int S = col / 16, kb = (col % 16) / 4, j = col % 4, tile = row / 16, lane = 16 * kb + row % 16;
                const size_t at = (((size_t)S * (N / 16) + tile) * 64 + lane) * 4 + j;
                CHECK(out[at] == W[(size_t)row * K + col]);
                seen[at]++;
            }
        for (int c : seen) CHECK(c == 1);
    }
}

static void test_lds_limit() {      // the flag is set by the first call; the device comes back
    DeviceOnce once{};
    CHECK(!once.done(0));
    CHECK(raise_lds_limit(once, {{(const void *)&g_failed, 1024}, {(const void *)&g_error, 2048}}) == 0);
    CHECK(once.done(0));
    CHECK(raise_lds_limit(once, {{(const void *)&g_failed, 1024}}) == 0);
    CHECK(device_cu_count(0) >= 1);
}

int main() {
    test_layout_and_upload();
    test_refused_allocation();
    test_arithmetic();
    test_lds_limit();
    if (g_failed) { fprintf(stderr, "host_pack_test: %d checks failed\n", g_failed); return 1; }
    puts("host_pack_test: ok");
    return 0;
}
