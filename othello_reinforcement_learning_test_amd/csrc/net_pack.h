// net_pack.h -- the host side the trunk files share: the fp16 hi/lo operand split and the power-of-two weight scale of the
// fp16-split kernels, the stem and Winograd weight transforms, device buffers that free themselves, and the once-per-
// (function, device) dynamic-LDS attribute.  Host code only: nothing here reaches a code object.
#pragma once
#include <math.h>
#include <string.h>

#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "net.h"

namespace oth {

// v = hi + lo, both f16 (~22 significant bits): the operand split of every fp16-split trunk
inline void split_f16(float v, uint16_t& hi, uint16_t& lo) {
    const _Float16 hh = (_Float16)v;
    const _Float16 ll = (_Float16)(v - (float)hh);
    memcpy(&hi, &hh, 2);
    memcpy(&lo, &ll, 2);
}

inline float max_abs(const std::vector<float>& w) {
    float mx = 0.f;
    for (float x : w) mx = fmaxf(mx, fabsf(x));
    return mx;
}

// The power of two that puts the largest |w| of a layer into [8192, 16384] (exponent clamped to +-24): the lo halves of
// the split then stay in the normal f16 range.  The direct packers take the maximum and the scale in float, the Winograd
// ones (whose U = G g is a float64 product) in double: two entries, so that each keeps its arithmetic to the bit.
inline float pow2_weight_scale(float mx) {
    int e = mx > 0.f ? (int)floorf(log2f(16384.0f / mx)) : 0;
    e = e > 24 ? 24 : (e < -24 ? -24 : e);
    return ldexpf(1.0f, e);
}
inline double pow2_weight_scale(double mx) {
    int e = mx > 0.0 ? (int)floor(log2(16384.0 / mx)) : 0;
    e = e > 24 ? 24 : (e < -24 ? -24 : e);
    return ldexp(1.0, e);
}

// The direct 3x3 stem as ONE k-step of v_mfma_f32_16x16x32_f16: gemm k = tap*3 + plane (27 of 32 used), wave wv owns
// output channels [16 wv, 16 wv + 16); lane l holds W[row = l&15][k = 8*(l>>4) + j].  out: [wave][hi, lo][64 lanes] x 16 B.
// Returns the weight scale.
inline float pack_stem_f16(const FoldedConv& stem, int waves, std::vector<uint16_t>& out) {
    const size_t frag = 64 * 8;   // halfs per fragment
    const float scale = pow2_weight_scale(max_abs(stem.w));
    out.assign((size_t)waves * 2 * frag, 0);
    for (int wv = 0; wv < waves; ++wv)
        for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) {
                const int k = 8 * (l >> 4) + j, co = 16 * wv + (l & 15);
                const float v = k < 27 ? stem.w[(size_t)k * stem.cout + co] * scale : 0.f;   // [tap][cin = 3][cout]
                uint16_t* hi = &out[(size_t)wv * 2 * frag + (size_t)l * 8 + j];
                split_f16(v, hi[0], hi[frag]);
            }
    return scale;
}

// 1-D Winograd F(2,3) weight transform along x of an F -> F 3x3 convolution, in float64:
//   U[dy][xi][ci][co] = sum_i G[xi][i] w[tap = 3 dy + i][ci][co],  G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1].  Returns max |U|.
inline double winograd_f23_U(const FoldedConv& cv, int F, std::vector<double>& U) {
    static const double G[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};
    U.resize((size_t)3 * 4 * F * F);
    double mx = 0.0;
    for (int d = 0; d < 3; ++d)
        for (int xi = 0; xi < 4; ++xi)
            for (int ci = 0; ci < F; ++ci)
                for (int co = 0; co < F; ++co) {
                    double u = 0.0;
                    for (int i = 0; i < 3; ++i) u += G[xi][i] * (double)cv.w[((size_t)(d * 3 + i) * F + ci) * F + co];
                    U[(((size_t)d * 4 + xi) * F + ci) * F + co] = u;
                    mx = fmax(mx, fabs(u));
                }
    return mx;
}

// A device allocation that frees itself.  The owner binds the device before it lets go (oth_net_destroy, net_free_device).
template <typename T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    int alloc(size_t bytes) {
        reset();
        OTH_HIP(hipMalloc(&p_, bytes));
        return OTH_OK;
    }
    template <typename V>
    int upload(const std::vector<V>& v) {   // the bytes of v, whatever T the kernel reads them as
        if (int rc = alloc(v.size() * sizeof(V))) return rc;
        OTH_HIP(hipMemcpy(p_, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice));
        return OTH_OK;
    }
    T* get() const { return p_; }

  private:
    T* p_ = nullptr;
};

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the (function, device) pair: set once for each
inline int set_max_dynamic_lds(const void* kernel, int device, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({kernel, device})) return OTH_OK;
    OTH_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.insert({kernel, device});
    return OTH_OK;
}

}  // namespace oth
