// TEST INFRASTRUCTURE: a stand-alone program over pack_conv_planes of patch2pix_amd/csrc/host_pack.h (the weight planes of
// P2P_REGRESS_GENERIC_FP16X2), compiled against the HIP stand-in of this directory with -fsanitize=address,undefined
// (tests/test_generic_mode_host.py).  It launches no kernel: it packs convolution weights of a few shapes -- co past and short
// of the 32-column tiles, input channels that are no multiple of 16, 1 / 9 / 25 taps -- into exactly sized buffers, decodes
// every entry of the stream and compares it with a direct evaluation, uploads the stream as the blob regress_generic_h2.hip
// builds, and refuses an allocation.  Exit status 0 and "generic_pack_test: ok" on success; the sanitizers report overruns,
// leaks and undefined behaviour on their own.
#include "../../patch2pix_amd/csrc/host_pack.h"

#include <cstdarg>
#include <cstring>

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

static double half_value(uint16_t u) { _Float16 h; memcpy(&h, &u, 2); return (double)(float)h; }

// weights whose magnitudes stay within 2^-12 of their channel's largest one: scaled to [2^11, 2^12) at the top they are >= 2^-1,
// so the low plane is a NORMAL fp16 or exact and hi + lo is the value to 2^-22 relative (a weight more than 2^14 below its
// channel's maximum is resolved to 2^-25 of 2^12 x that maximum instead, which the kernels' fp32 accumulation cannot tell apart)
static std::vector<float> make_weights(int co, int cin, int taps, unsigned seed) {
    std::vector<float> w((size_t)co * cin * taps);
    unsigned s = seed;
    for (size_t q = 0; q < w.size(); ++q) {
        s = s * 1664525u + 1013904223u;
        const int n = (int)(q / ((size_t)cin * taps));
        const float mant = 1.f + (float)(s >> 9) / (float)(1 << 23);               // [1, 2), 23 random bits
        const int e = -(int)((s >> 3) % 12) + (n % 7) - 3;                          // 12 binades, a different top per channel
        w[q] = std::ldexp((s & 4) ? -mant : mant, e);
        if ((s & 0x3f0) == 0) w[q] = 0.f;                                           // exact zeros among them
    }
    return w;
}

static void test_shape(int co, int cin, int ker, unsigned seed) {
    const int taps = ker * ker, ntiles = 2 * ((co + 63) / 64), nslab = (cin + 15) / 16;
    const std::vector<float> w = make_weights(co, cin, taps, seed);
    const size_t halfs = conv_planes_halfs(cin, taps, ntiles);
    CHECK(halfs == (size_t)nslab * taps * ntiles * 1024);
    std::vector<uint16_t> out(halfs, 0x7e00);                                       // NaNs: every entry must be written
    std::vector<int> texp(co, 99);
    pack_conv_planes(w.data(), co, cin, taps, ntiles, out.data(), texp.data());
    for (int n = 0; n < co; ++n) {                                                  // the exponent: the channel's top in [2^11, 2^12)
        double mx = 0.0;
        for (size_t q = 0; q < (size_t)cin * taps; ++q) mx = std::max(mx, std::fabs((double)w[(size_t)n * cin * taps + q]));
        CHECK(mx > 0.0 && std::ldexp(mx, texp[n]) >= 2048.0 && std::ldexp(mx, texp[n]) < 4096.0);
    }
    std::vector<int> seen((size_t)co * cin * taps, 0);
    for (int sl = 0; sl < nslab; ++sl)
        for (int tap = 0; tap < taps; ++tap)
            for (int t = 0; t < ntiles; ++t)
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < 8; ++i) {
                        const size_t at = ((((size_t)sl * taps + tap) * ntiles + t) * 2 * 64 + lane) * 8 + i;
                        const uint16_t hi = out[at], lo = out[at + 512];
                        const int n = 32 * t + (lane & 31), chn = 16 * sl + 8 * (lane >> 5) + i;
                        if (n >= co || chn >= cin) {                                // zero fill past co and past the real channels
                            CHECK(hi == 0 && lo == 0);
                            continue;
                        }
                        const size_t src = ((size_t)n * cin + chn) * taps + tap;
                        const double want = (double)w[src], got = std::ldexp(half_value(hi) + half_value(lo), -texp[n]);
                        CHECK(std::fabs(got - want) <= std::ldexp(std::fabs(want), -22));
                        CHECK(std::fabs(half_value(hi)) <= 4096.0);                 // (a value just below 2^12 rounds up to it)
                        seen[src]++;
                    }
    for (int c : seen) CHECK(c == 1);

    // the blob of a layer as regress_generic_h2.hip lays it out: the stream + one step of zeros, then the folded scales
    DeviceBlob b;
    const size_t ow = b.take<unsigned char>((halfs + (size_t)ntiles * 1024) * sizeof(uint16_t)), os = b.take<float>(co);
    pack_conv_planes(w.data(), co, cin, taps, ntiles, (uint16_t *)b.at<unsigned char>(ow), texp.data());
    for (int n = 0; n < co; ++n) b.at<float>(os)[n] = std::ldexp(1.f, -texp[n]);
    g_error[0] = 0;
    hipemu::refuse_allocs = 1;
    CHECK(b.upload("refused planes") == P2P_ENOMEM && !b.uploaded() && hipemu::refuse_allocs == 0);
    CHECK(strstr(g_error, "refused planes") != nullptr);
    DeviceBlob again;                                                               // the caller's retry: a fresh blob
    const size_t ow2 = again.take<unsigned char>((halfs + (size_t)ntiles * 1024) * sizeof(uint16_t));
    pack_conv_planes(w.data(), co, cin, taps, ntiles, (uint16_t *)again.at<unsigned char>(ow2), texp.data());
    CHECK(again.upload("planes") == P2P_OK && again.uploaded());
    CHECK(memcmp(again.dev<unsigned char>(ow2), out.data(), halfs * sizeof(uint16_t)) == 0);
    const unsigned char *tail = again.dev<unsigned char>(ow2) + halfs * sizeof(uint16_t);
    for (size_t q = 0; q < (size_t)ntiles * 2048; ++q) CHECK(tail[q] == 0);          // the step the prefetch runs into
}

int main() {
    test_shape(32, 6, 3, 1);          // case B: 6 real channels in a slab of 16, co short of the 64-column pair
    test_shape(48, 67, 3, 2);         // co no multiple of 32, channels 64 + 3
    test_shape(16, 24, 1, 3);         // 1x1
    test_shape(80, 16, 5, 4);         // 5x5, three column tiles used of four
    {   // a channel of zeros: exponent 0, planes of zeros
        std::vector<float> w(2 * 16 * 9, 0.f);
        for (int q = 0; q < 16 * 9; ++q) w[q] = 0.25f;
        std::vector<uint16_t> out(conv_planes_halfs(16, 9, 2), 1);
        int texp[2] = {7, 7};
        pack_conv_planes(w.data(), 2, 16, 9, 2, out.data(), texp);
        CHECK(texp[0] == 13 && texp[1] == 0);                                       // 0.25 x 2^13 = 2^11
        CHECK(half_value(out[0]) == 2048.0 && out[512] == 0 && out[8 * 1] == 0);    // lane 1 = output channel 1: zeros
    }
    if (g_failed) { fprintf(stderr, "generic_pack_test: %d checks failed\n", g_failed); return 1; }
    puts("generic_pack_test: ok");
    return 0;
}
