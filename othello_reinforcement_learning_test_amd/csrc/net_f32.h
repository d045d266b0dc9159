// net_f32.h -- what the two exact-fp32 MFMA trunks share: net_f32.hip (k_trunk_f32: one wave carries a position group
// through the whole network) and net_f32c.hip (k_trunk_f32c: the waves of a workgroup share a position group and split
// the output channels -- the widths whose accumulators do not fit one wave).
#pragma once
#include <vector>

#include "net_pack.h"

namespace oth {

using f32x4 = float __attribute__((ext_vector_type(4)));

struct F32Weights {
    DevBuf<float4> w;      // [layer][k-step][chunk][64 lanes] x 16 B (k_trunk_f32; null where only k_trunk_f32c runs)
    DevBuf<float4> wc;     // [layer][wave][k-step][chunk][64 lanes] x 16 B (k_trunk_f32c; null where it has no build)
    DevBuf<float> bias;    // [layers][F]
    std::vector<uint32_t> layer_off;    // in float4 units, into w
    std::vector<uint32_t> layer_off_c;  // in float4 units, into wc
};

struct F32Args {
    const float4* w;
    uint32_t layer_off[kMaxTrunkLayers];
    const float* bias;
    int n_layers;  // 1 + 2*blocks
    HeadParams heads;
    const float* pfc_wt;
    const float* vfc1_wt;
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int F, int BS, int P>
struct TrunkGeom {
    static constexpr int NB = F / 16;               // 16-channel row blocks
    static constexpr int CELLS = BS * BS;
    static constexpr int NP = CELLS + 1;            // policy outputs (pass included)
    static constexpr int NC = P * CELLS;            // output cells of a position group
    static constexpr int T = (NC + 15) / 16;        // 16-cell tiles
    static constexpr int PW = BS + 2;               // padded row
    static constexpr int POSW = PW * PW;            // padded plane of one position (words)
    static constexpr int PS = P * POSW;             // plane stride (words)
    static constexpr int NPL = F < 4 ? 4 : F;       // planes (the stem reads 4: self, opp, legal, zero)
    static constexpr int NW = 9 * NB;               // weight values per lane per k-step
    static constexpr int NCH = (NW + 3) / 4;        // 16-byte chunks per lane per k-step
    static constexpr int SCRATCH = 192 * P;         // head scratch (words) per position: pf0[64] pf1[64] vf[64]
    static constexpr int WAVE_WORDS = NPL * PS + SCRATCH;
};

// ---- net_f32c.hip
// waves per workgroup of k_trunk_f32c at `filters` (0: no build); each wave owns ceil(filters / 16 / waves) row blocks
int f32c_waves(int filters);
// true when a launch on `net` runs k_trunk_f32c: the widths only it serves, or OTH_F32_COOP=1 (read per call: the A/B
// switch) where both kernels have a build
bool f32c_selected(const oth_net* net);
// the fragment-ordered weights of k_trunk_f32c -> fw->wc (called by f32_pack)
int f32c_pack_weights(oth_net* net, F32Weights* fw);
int f32c_forward(oth_net* net, const F32Weights* fw, F32Args& a, const uint64_t* self_b, const uint64_t* opp_b, const uint64_t* legal, int64_t n,
                 const int32_t* n_valid, float* logp, float* v, hipStream_t stream);

}  // namespace oth
