// net.h -- the evaluator object and the trunk table.  net.hip owns the API, the weight folding, the head parameters and
// the table's rows in priority order; every trunk file (net_f32.hip with net_f32c.hip, net_wino6.hip, net_wino.hip,
// net_h3.hip, net_mfma.hip) defines one TrunkImpl row: its kernels, weight packing, launch and what kernel_info reports.
// net_pack.h holds the host helpers the packers share.
#pragma once
#include <vector>

#include "common.h"

namespace oth {

// One conv+BN pair folded for inference (eval-mode BN, reference L19):
//   y = conv(x, w) * scale + shift,  scale = gamma / sqrt(var + eps),  shift = beta - mean * scale
// stored as w'[tap][cin][cout] = w * scale[cout] and bias[cout] = shift.
struct FoldedConv {
    int cin = 0, cout = 0, taps = 0;
    std::vector<float> w;     // [taps][cin][cout]
    std::vector<float> bias;  // [cout]
};

constexpr int kMaxTrunkLayers = 48;  // 1 + 2*blocks

struct HostNet {
    int blocks = 0, filters = 0, board = 8;
    FoldedConv stem;               // 3 -> F, 3x3            (net.py:168)
    std::vector<FoldedConv> res;   // 2*blocks, F -> F, 3x3  (net.py:171-173)
    FoldedConv pconv, vconv;       // 1x1 heads              (net.py:76, 111)
    std::vector<float> pfc_w, pfc_b;    // [cells+1][2*cells], [cells+1]   (net.py:81; 8x8: [65][128])
    std::vector<float> vfc1_w, vfc1_b;  // [256][cells], [256]             (net.py:116)
    std::vector<float> vfc2_w, vfc2_b;  // [256], [1]        (net.py:117)
};

// device-side parameter block of the heads (fp32, shared by every trunk kernel)
struct HeadParams {
    const float* pconv_w;  // [F][2]
    const float* pconv_b;  // [2]
    const float* vconv_w;  // [F]
    const float* vconv_b;  // [1]
    const float* pfc_w;    // [65][128]
    const float* pfc_b;    // [65]
    const float* vfc1_w;   // [256][64]
    const float* vfc1_b;   // [256]
    const float* vfc2_w;   // [256]
    const float* vfc2_b;   // [1]
};

// One row of the trunk table (net.hip: kTrunks).  oth_net_load_state takes the first row that serves the network, packs
// that row's weights only and keeps the row; oth_net_forward_bits and oth_net_kernel_info call through it.
struct TrunkImpl {
    // does this trunk run `net` at `precision` (OTH_PREC_*)?  Reads the A/B switch of its row, if it has one.
    bool (*serves)(const oth_net* net, int precision);
    // weights in the kernel's fragment order -> net->trunk_w (set before the first upload: destroy frees a partial pack)
    int (*pack)(oth_net* net);
    void (*destroy)(void* weights);
    int (*forward)(oth_net* net, const uint64_t* self_b, const uint64_t* opp_b, const uint64_t* legal, int64_t n,
                   const int32_t* n_valid, float* logp, float* v, hipStream_t stream);
    // the kernel a launch of n positions runs, MFMA FLOPs issued per algorithmic FLOP, activation clamp (0: none)
    void (*info)(const oth_net* net, int64_t n, const char** name, double* issued_per_flop, double* clamp);
};
// the rows (function-local constants: a namespace-scope const object of host function pointers would be emitted for the device too)
const TrunkImpl* trunk_f32();    // net_f32.hip: exact fp32 (k_trunk_f32 / k_trunk_f32c), any width, 8x8 and 6x6
const TrunkImpl* trunk_wino6();  // net_wino6.hip: 1-D Winograd F(2,3), 64 filters on 6x6 (BASELINE configs[4])
const TrunkImpl* trunk_wino();   // net_wino.hip: 1-D Winograd F(2,3), 128 filters on 8x8
const TrunkImpl* trunk_h3();     // net_h3.hip: direct 3x3, one wave per position group (32 / 64 filters, 128 on 6x6)
const TrunkImpl* trunk_mfma();   // net_mfma.hip: direct 3x3, 128 filters on 8x8 (k_trunk16, three builds)

}  // namespace oth

struct oth_net {
    int device = 0;      // HIP device the weights live on (the creating thread's current device)
    int blocks = 0, filters = 0, board = 8;
    int precision = -1;  // OTH_PREC_*; -1 = no weights loaded
    oth::HostNet host;
    float* d_heads = nullptr;  // one allocation: the fp32 head parameters (shared by every trunk kernel)
    // the head FCs transposed so that lanes read consecutive outputs (net_heads_wave.h, k_trunk_w's heads_block2): an
    // allocation each, for every trunk whose Args carry them
    float* d_pfc_wt = nullptr;   // [2*cells][cells+1]
    float* d_vfc1_wt = nullptr;  // [cells][256]
    int* d_sat = nullptr;      // device flag: an fp16-split trunk kernel clamped an activation (oth_net_saturated)
    // Activations of the fp16-split trunks are carried PRE-SCALED by act_scale (a power of two, 16 by default: it keeps the
    // lo parts of the operand split clear of the f16 subnormals) and clamped at the f16 range of that scaled value; the
    // reference's fp32 forward has no clamp.  The scale enters a launch through the stem's input planes, the biases
    // (dev = host x act_scale: the arrays registered below) and the heads' un-scaling, so it is a RUN-TIME value:
    // oth_net_set_act_scale halves it when a launch saturated (range 1875 -> 30 000 at scale 1 in the Winograd trunks).
    float act_scale = 16.0f;
    struct ScaledBias { float* dev; std::vector<float> host; };
    std::vector<ScaledBias> scaled_bias;
    oth::HeadParams heads{};
    const oth::TrunkImpl* trunk = nullptr;  // the row that serves this network at `precision`
    void* trunk_w = nullptr;                // its packed weights (the row's own struct)
};

// The in-place MFMAs of net_mfma.hip / net_h3.hip are inline asm: hipcc inserts no wait states between a VALU write of a
// VGPR and an asm MFMA reading it (2 needed on gfx90a+).  Accumulators are zeroed by VALU moves which the compiler likes to
// sink next to their first use; OTH_PIN_ACC keeps the move of one accumulator in front of this point and
// OTH_PIN_ACC_END supplies the wait states once for all of them.  tools/check_mfma_hazards.py checks the built objects.
#define OTH_PIN_ACC(x) asm volatile("" : "+v"(x))
#define OTH_PIN_ACC_END()                  \
    do {                                   \
        asm volatile("s_nop 1" ::: "memory"); \
        __builtin_amdgcn_sched_barrier(0); \
    } while (0)

namespace oth {
// upload host x net->act_scale to dev and keep both for oth_net_set_act_scale (dev stays owned by the caller's weight struct)
int register_scaled_bias(oth_net* net, float* dev, std::vector<float> host);   // net.hip
}  // namespace oth
