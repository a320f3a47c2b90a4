// Host side of every handle, written once: the device allocation behind a handle's packed weights (DeviceBlob), the arithmetic
// that goes into those blobs (BatchNorm fold, fp32 -> two fp16 planes, power-of-two channel exponents, FC weights as MFMA
// fragments) and what every launcher with a large dynamic LDS allocation does once per device (raise_lds_limit).  Host code
// only: included where weights are packed or such a kernel is launched, not from p2p_common.h.
#pragma once
#include "p2p_common.h"
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <utility>
#include <vector>

namespace p2p {

// One device allocation made of aligned parts.  take() lays the parts out (all of them, before anything is filled in), at() is
// the zero-filled host staging copy a packer writes, upload() is the one hipMalloc + hipMemcpy, dev() the device address of a
// part afterwards.  The blob owns the allocation: a handle holds its blob(s) by value, so `delete handle` frees them.
class DeviceBlob {
public:
    DeviceBlob() = default;
    DeviceBlob(const DeviceBlob &) = delete;
    DeviceBlob &operator=(const DeviceBlob &) = delete;
    DeviceBlob(DeviceBlob &&o) noexcept : host_(std::move(o.host_)), dev_(o.dev_), bytes_(o.bytes_) { o.dev_ = nullptr; o.bytes_ = 0; }
    DeviceBlob &operator=(DeviceBlob &&o) noexcept {
        if (this != &o) {
            release();
            host_ = std::move(o.host_); dev_ = o.dev_; bytes_ = o.bytes_;
            o.dev_ = nullptr; o.bytes_ = 0;
        }
        return *this;
    }
    ~DeviceBlob() { release(); }

    // a part of `count` elements of T, padded to 64 elements (256 bytes for the fp32 parts); returns where it starts, in elements
    // of T from the start of the blob
    template <class T> size_t take(size_t count) {
        const size_t off = bytes_ / sizeof(T);
        bytes_ += ((count + 63) & ~size_t(63)) * sizeof(T);
        return off;
    }
    size_t bytes() const { return bytes_; }
    template <class T> T *at(size_t off) {                  // host staging copy (zeros until written), valid until upload()
        if (host_.size() < bytes_) host_.resize(bytes_, 0);
        return (T *)host_.data() + off;
    }
    template <class T> const T *dev(size_t off = 0) const { return (const T *)dev_ + off; }     // after upload()
    bool uploaded() const { return dev_ != nullptr; }

    // P2P_ENOMEM when the allocation fails, P2P_EHIP when the copy does (nothing stays allocated either way)
    int upload(const char *what) {
        at<unsigned char>(0);
        hipError_t e = hipMalloc(&dev_, bytes_);
        if (e != hipSuccess) {
            dev_ = nullptr;
            set_error("%s: hipMalloc of %zu bytes failed: %s", what, bytes_, hipGetErrorString(e));
            return P2P_ENOMEM;
        }
        e = hipMemcpy(dev_, host_.data(), bytes_, hipMemcpyHostToDevice);
        std::vector<unsigned char>().swap(host_);
        if (e != hipSuccess) {
            release();
            set_error("%s: hipMemcpy of %zu bytes failed: %s", what, bytes_, hipGetErrorString(e));
            return P2P_EHIP;
        }
        return P2P_OK;
    }
    void release() {                                        // harmless on a blob that was never uploaded, and twice
        if (dev_) (void)hipFree(dev_);
        dev_ = nullptr;
    }

private:
    std::vector<unsigned char> host_;
    unsigned char *dev_ = nullptr;
    size_t bytes_ = 0;
};

// eval-mode BatchNorm (eps 1e-5) as y = x * scale + shift
static inline void fold_bn(const p2p_bn_params &bn, int n, float *scale, float *shift) {
    for (int i = 0; i < n; ++i) {
        const float inv = 1.0f / std::sqrt(bn.running_var[i] + 1e-5f);
        const float a = bn.weight[i] * inv;
        scale[i] = a;
        shift[i] = bn.bias[i] - bn.running_mean[i] * a;
    }
}

// fp32 -> two fp16 planes: v = hi + lo to within 2^-24 |v| (both round to nearest even, like the kernels' own splits)
static inline void split_fp16_planes(float v, uint16_t *hi, uint16_t *lo) {
    const _Float16 h = (_Float16)v;
    *hi = __builtin_bit_cast(uint16_t, h);
    *lo = __builtin_bit_cast(uint16_t, (_Float16)(v - (float)h));
}

// fp32 -> ONE fp16 (round to nearest even): the single-plane operand of P2P_REGRESS_FP16, relative error <= 2^-11 inside the
// normal range of fp16
static inline uint16_t round_fp16(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }

// the exponent t for which mx * 2^t lies in [2^(target-1), 2^target): with target 12 the exact scaling that brings a channel's
// largest weight magnitude mx to the top of the fp16 range the planes resolve (undone in the folded BatchNorm scale); 0 for a
// channel of zeros or with a non-finite weight
static inline int pow2_exponent_to(double mx, int target) {
    if (!(mx > 0.0) || !std::isfinite(mx)) return 0;
    int e;
    std::frexp(mx, &e);          // mx = m * 2^e, m in [0.5, 1)
    return target - e;
}

// fc weight [n][k] (row-major, torch Linear; n, k multiples of 16) -> B fragments of v_mfma_f32_16x16x4_f32 in the K order of
// fc_batch_parse / gen_fc_kernel: out[((S * (n / 16) + tile) * 64 + lane) * 4 + j] = W[16 tile + (lane & 15)][16 S + 4 (lane >> 4) + j]
static inline void pack_fc_mfma(const float *w, int n, int k, float *out) {
    for (int S = 0; S < k / 16; ++S)
        for (int t = 0; t < n / 16; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j)
                    out[(((size_t)S * (n / 16) + t) * 64 + lane) * 4 + j] = w[(size_t)(16 * t + (lane & 15)) * k + 16 * S + 4 * (lane >> 4) + j];
}

// conv weight [co][cin][taps] (torch Conv2d, taps = k * k) -> the two-plane fp16 B fragments of v_mfma_f32_32x32x16_f16 in the
// order regress_generic_h2.hip streams them, K in slabs of 16 input channels, slabs outer:
//   out[((((slab * taps + tap) * ntiles + t) * 2 + plane) * 64 + lane) * 8 + i] = plane (0 high, 1 low) of
//   W[n = 32 t + (lane & 31)][16 slab + 8 (lane >> 5) + i][tap] * 2^texp[n],      texp[n] = pow2_exponent_to(max |W[n]|, 12),
// zeros past co and past cin (the last slab of a cin that is no multiple of 16).  conv_planes_halfs: fp16 values of the stream.
static inline size_t conv_planes_halfs(int cin, int taps, int ntiles) { return (size_t)((cin + 15) / 16) * taps * ntiles * 1024; }
static inline void pack_conv_planes(const float *w, int co, int cin, int taps, int ntiles, uint16_t *out, int *texp) {
    const int nslab = (cin + 15) / 16;
    for (int n = 0; n < co; ++n) {
        double mx = 0.0;
        for (size_t q = 0; q < (size_t)cin * taps; ++q) mx = std::max(mx, (double)std::fabs(w[(size_t)n * cin * taps + q]));
        texp[n] = pow2_exponent_to(mx, 12);
    }
    for (int sl = 0; sl < nslab; ++sl)
        for (int tap = 0; tap < taps; ++tap)
            for (int t = 0; t < ntiles; ++t)
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < 8; ++i) {
                        const int n = 32 * t + (lane & 31), chn = 16 * sl + 8 * (lane >> 5) + i;
                        uint16_t hi = 0, lo = 0;
                        if (n < co && chn < cin) split_fp16_planes(std::ldexp(w[((size_t)n * cin + chn) * taps + tap], texp[n]), &hi, &lo);
                        const size_t at = ((((size_t)sl * taps + tap) * ntiles + t) * 2 * 64 + lane) * 8 + i;
                        out[at] = hi;
                        out[at + 512] = lo;
                    }
}

// Conv4d weight in the stored layout [k(da)][co][ci][k(db)][k(dc)][k(dd)] (co, ci <= 16) -> the two-plane fp16 B fragments of
// v_mfma_f32_16x16x32_f16 in the order consensus_generic_h2.hip streams them: per da slice, steps of 4 / nh taps of the slice's
// k^3 in the order (db, dc, dd), nh = 1 (8 staged input channels) or 2 (16):
//   out[(((da * nstep + step) * 2 + plane) * 64 + lane) * 8 + i] = plane (0 high, 1 low) of
//   W[n = lane & 15][ch = 8 ((lane >> 4) % nh) + i][da][tap = (4 / nh) step + (lane >> 4) / nh] * 2^texp[n],
//   texp[n] = pow2_exponent_to(max |W[n]|, 12), zeros past co, past ci and past the slice's last tap.
// Branch 1 is the transposed branch of symmetric_mode: in the volume's own coordinates the weight of offset (da, db, dc, dd) is
// W[dc][dd][da][db] (the exponents are those of branch 0: the same values).
static inline size_t conv4d_planes_steps(int k, int nh) { return (size_t)(k * k * k + 4 / nh - 1) / (4 / nh); }
static inline size_t conv4d_planes_halfs(int k, int nh) { return (size_t)k * conv4d_planes_steps(k, nh) * 1024; }
static inline void pack_conv4d_planes(const float *w, int k, int co, int ci, int nh, int br, uint16_t *out, int *texp) {
    const int ntap = k * k * k, tpm = 4 / nh, nstep = (int)conv4d_planes_steps(k, nh);
    auto W = [&](int o, int i, int da, int db, int dc, int dd) {
        return w[((((size_t)(da * co + o) * ci + i) * k + db) * k + dc) * k + dd];
    };
    for (int n = 0; n < co; ++n) {
        double mx = 0.0;
        for (int i = 0; i < ci; ++i)
            for (int da = 0; da < k; ++da)
                for (int t = 0; t < ntap; ++t) mx = std::max(mx, (double)std::fabs(W(n, i, da, t / (k * k), (t / k) % k, t % k)));
        texp[n] = pow2_exponent_to(mx, 12);
    }
    for (int da = 0; da < k; ++da)
        for (int s = 0; s < nstep; ++s)
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < 8; ++i) {
                    const int n = lane & 15, g = lane >> 4, tap = tpm * s + g / nh, ch = 8 * (g % nh) + i;
                    uint16_t hi = 0, lo = 0;
                    if (n < co && ch < ci && tap < ntap) {
                        const int db = tap / (k * k), dc = (tap / k) % k, dd = tap % k;
                        split_fp16_planes(std::ldexp(br ? W(n, ch, dc, dd, da, db) : W(n, ch, da, db, dc, dd), texp[n]), &hi, &lo);
                    }
                    const size_t at = (((size_t)da * nstep + s) * 2 * 64 + lane) * 8 + i;
                    out[at] = hi;
                    out[at + 512] = lo;
                }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
// What a launcher does before a kernel whose dynamic LDS allocation exceeds the default limit: ask for the current device (once
// per launch) and, on that device's first launch, raise the limit of each kernel; `once` is set only after all of them succeeded.
// Returns the device (>= 0) or P2P_EHIP.
struct LdsLimit { const void *kernel; int bytes; };
static inline int raise_lds_limit(DeviceOnce &once, std::initializer_list<LdsLimit> kernels) {
    int dev = 0;
    P2P_HIP_CHECK(hipGetDevice(&dev));
    if (!once.done(dev)) {
        for (const LdsLimit &k : kernels) P2P_HIP_CHECK(hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes));
        once.set(dev);
    }
    return dev;
}

// compute units of a device (>= 1; the grids of the persistent kernels), asked once per device and process; P2P_EHIP (< 0) if the
// runtime refuses
static inline int device_cu_count(int dev) {
    static std::atomic<int> cus[64];
    const bool slot = dev >= 0 && dev < 64;
    int ncu = slot ? cus[dev].load(std::memory_order_relaxed) : 0;
    if (ncu > 0) return ncu;
    P2P_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    ncu = std::max(ncu, 1);
    if (slot) cus[dev].store(ncu, std::memory_order_relaxed);
    return ncu;
}

}  // namespace p2p
