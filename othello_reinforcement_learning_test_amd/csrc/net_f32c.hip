// net_f32c.hip -- OthelloResNet forward in exact fp32 on the matrix cores for the WIDE trunks (144 to 256 filters, 8x8 and
// 6x6): the workgroup-cooperative form of net_f32.hip's k_trunk_f32.
//
// Why a second kernel: k_trunk_f32 gives one wave a whole position group and ALL output channels -- NB x T accumulators
// plus as many residual registers per lane.  At 128 filters on 8x8 that is 2 x 8 x 4 x 4 = 256 of the 512 registers a
// lane can have; at 256 filters it would be 512 before the first weight fragment.
//
// Design:
//   * W waves of ONE workgroup share the activation planes of P positions in LDS -- the layout of k_trunk_f32,
//     [channel][position][(BS+2) x (BS+2) cells] with a zero border, so a 3x3 tap stays a constant address offset.
//   * each wave owns NBW = ceil(NB / W) consecutive 16-channel row blocks of the OUTPUT: their accumulators and their
//     residual stay in its registers for the whole network (NBW x T of each; 4 x 4 at 256 filters on 8x8 -- the tile
//     shape of k_trunk_f32<64, 8, 1, 4>), and it streams only its own slice of the fragment-ordered weights from L2
//     (host packing: [layer][wave][k-step][chunk][lane]).
//   * per layer: every wave reads all the input planes; workgroup barrier; every wave rewrites the planes of its own
//     row blocks in place (bias, skip, ReLU); workgroup barrier.  Two barriers per layer is the whole cost of sharing.
//   * NB that W does not divide (176 filters = 11 row blocks on 4 waves): the packed weights of the missing row blocks
//     are zero and their stores are skipped -- the code of a wave does not depend on how many of its blocks are real.
//   * every barrier is on workgroup-uniform control flow: the only early exit (a workgroup past n_valid) is above the
//     first one, and the layer count is a kernel argument.
//   * each output channel is summed in k_trunk_f32's order -- k-steps of four input channels, the nine taps inside a
//     step, then bias, skip, ReLU -- and the heads are the same heads_wave_n, one wave per position: where both kernels
//     have a build (OTH_F32_COOP=1 routes 64 and 128 filters here) their outputs agree bit for bit.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "net_f32.h"
#include "net_heads_wave.h"

namespace oth {

template <int F, int BS, int P, int W>
__global__ __launch_bounds__(64 * W) void k_trunk_f32c(F32Args a, const uint64_t* __restrict__ sb,
                                                         const uint64_t* __restrict__ ob,
                                                         const uint64_t* __restrict__ lgl, int64_t n,
                                                         const int32_t* __restrict__ n_valid,
                                                         float* __restrict__ logp, float* __restrict__ vout) {
    using G = TrunkGeom<F, BS, P>;
    constexpr int NB = G::NB, CELLS = G::CELLS, NP = G::NP, NC = G::NC, T = G::T, PW = G::PW, POSW = G::POSW, PS = G::PS;
    constexpr int NBW = (NB + W - 1) / W;        // row blocks of a wave (the last wave's may lie beyond NB: zero weights)
    constexpr int NCH = (9 * NBW + 3) / 4;       // 16-byte chunks per lane per k-step
    static_assert(P <= W, "one wave per position in the heads");
    extern __shared__ __attribute__((aligned(16))) float lds_f32c[];
    int64_t nv = n;
    if (n_valid) {
        const int64_t k = *n_valid;
        nv = k < n ? k : n;
    }
    const int64_t pos0 = (int64_t)blockIdx.x * P;
    if (pos0 >= nv) return;   // the whole workgroup: above the first barrier
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n16 = lane & 15, kg = lane >> 4;
    float* act = lds_f32c;
    float* scratch = act + G::NPL * PS;

    // ---- planes (shared work): zero everything (borders stay zero for the whole network), then the three input planes
    for (int i = threadIdx.x; i < G::NPL * PS; i += 64 * W) act[i] = 0.f;
    __syncthreads();
    if (wave < P && pos0 + wave < nv && lane < CELLS) {
        const uint64_t b0 = sb[pos0 + wave], b1 = ob[pos0 + wave], b2 = lgl[pos0 + wave];
        const int off = wave * POSW + (lane / BS + 1) * PW + (lane % BS + 1);
        act[0 * PS + off] = (b0 >> lane) & 1ULL ? 1.f : 0.f;   // get_tensor_input planes (bitboard.pyx:309-323)
        act[1 * PS + off] = (b1 >> lane) & 1ULL ? 1.f : 0.f;
        act[2 * PS + off] = (b2 >> lane) & 1ULL ? 1.f : 0.f;
    }
    __syncthreads();

    // ---- per-lane tile geometry: padded-plane offset of this lane's cell in tile t (+ its k-group plane for reads)
    int rd_off[T], wr_off[T];
    bool valid[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int ci = t * 16 + n16;
        valid[t] = ci < NC;
        const int c = valid[t] ? ci : 0;
        const int p = c / CELLS, r = c % CELLS;
        const int cell = p * POSW + (r / BS + 1) * PW + (r % BS + 1);
        rd_off[t] = cell + kg * PS;          // B operand: input channel 4*kc + kg
        wr_off[t] = cell + 4 * kg * PS;      // D rows: output channel 16*blk + 4*kg + r
    }
    const int blk0 = wave * NBW;             // this wave's first row block

    f32x4 acc[NBW][T], res[NBW][T];
#pragma unroll
    for (int b = 0; b < NBW; ++b)
#pragma unroll
        for (int t = 0; t < T; ++t) {
            acc[b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            res[b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

    for (int layer = 0; layer < a.n_layers; ++layer) {
        const int KC = layer == 0 ? 1 : F / 4;   // k-steps of 4 input channels (stem: 3 planes + a zero plane)
        const float4* wl = a.w + a.layer_off[layer] + (size_t)wave * KC * NCH * 64 + lane;   // + (kc*NCH + chunk)*64
        float4 wq[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) wq[c] = wl[(size_t)c * 64];
        float4 bias_q[NBW];   // the epilogue's biases, requested before the convolution
#pragma unroll
        for (int b = 0; b < NBW; ++b)
            bias_q[b] = blk0 + b < NB ? *(const float4*)(a.bias + (size_t)layer * F + (blk0 + b) * 16 + 4 * kg)
                                      : float4{0.f, 0.f, 0.f, 0.f};
        for (int kc = 0; kc < KC; ++kc) {
            float w[NCH * 4];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                w[4 * c + 0] = wq[c].x; w[4 * c + 1] = wq[c].y; w[4 * c + 2] = wq[c].z; w[4 * c + 3] = wq[c].w;
            }
            {   // request the next k-step's fragments (the last step re-reads its own: harmless)
                const int kn = kc + 1 < KC ? kc + 1 : kc;
#pragma unroll
                for (int c = 0; c < NCH; ++c) wq[c] = wl[((size_t)kn * NCH + c) * 64];
            }
            const float* src = act + kc * 4 * PS;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int toff = (tap / 3 - 1) * PW + (tap % 3 - 1);
                float bv[T];
#pragma unroll
                for (int t = 0; t < T; ++t) bv[t] = src[rd_off[t] + toff];
#pragma unroll
                for (int b = 0; b < NBW; ++b)
#pragma unroll
                    for (int t = 0; t < T; ++t) acc[b][t] = mfma4(w[tap * NBW + b], bv[t], acc[b][t]);
            }
        }
        __syncthreads();   // every wave has read the planes of this layer's input
        // ---- epilogue: bias, skip connection (net.py:58-59), ReLU; rewrite the planes of this wave's row blocks in place
        const bool add_res = layer > 0 && (layer & 1) == 0;   // second conv of a block
        const bool set_res = layer == 0 || add_res;
#pragma unroll
        for (int b = 0; b < NBW; ++b) {
            const float4 bias = bias_q[b];
            const bool real = blk0 + b < NB;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                f32x4 v = acc[b][t];
                v[0] += bias.x; v[1] += bias.y; v[2] += bias.z; v[3] += bias.w;
                if (add_res) v += res[b][t];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                if (set_res) res[b][t] = v;
                acc[b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (real && valid[t]) {
                    float* dst = act + ((blk0 + b) * 16) * PS + wr_off[t];
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[r * PS] = v[r];
                }
            }
        }
        __syncthreads();   // the planes hold this layer's output
    }

    // ---- heads (net.py:62-136): wave p takes position p, from the shared planes; a dead position is computed, not stored
    if (wave < P) {
        const int c = lane < CELLS ? lane : 0;
        const float* const srcs[1] = {act + wave * POSW + (c / BS + 1) * PW + (c % BS + 1)};
        float* const lps[1] = {logp + (pos0 + wave) * NP};
        float* const vs[1] = {vout + pos0 + wave};
        const bool live[1] = {pos0 + wave < nv};
        heads_wave_n<F, BS, 1>(a.heads, a.pfc_wt, a.vfc1_wt, srcs, PS, scratch + wave * 192, lane, lps, vs, live);
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
int f32c_waves(int F) {
    switch (F) {
        case 64: case 128: case 160: return 2;   // 2 / 4 / 5 row blocks per wave
        case 144: return 3;                      // 3
        case 176: case 192: case 208: case 224: case 240: case 256: return 4;   // 3 (176: one padded) / 3 / 4 (208, 224, 240: padded) / 4
        default: return 0;
    }
}

bool f32c_selected(const oth_net* net) {
    if (!f32c_waves(net->filters)) return false;
    if (net->filters > 128) return true;
    const char* e = getenv("OTH_F32_COOP");
    return e && atoi(e) == 1;
}

// FoldedConv weights are [tap][cin][cout]; lane l of wave wv, k-step kc needs, for e = tap*NBW + j,
// W[cout = 16*(wv*NBW + j) + (l & 15)][cin = 4*kc + (l >> 4)][tap]  (cin >= c.cin or cout >= F: zero)
static void pack_layer_c(const FoldedConv& c, int F, int W, int kc_steps, std::vector<float>& out) {
    const int NB = F / 16, NBW = (NB + W - 1) / W, NW = 9 * NBW, NCH = (NW + 3) / 4;
    const size_t base = out.size();
    out.resize(base + (size_t)W * kc_steps * NCH * 64 * 4, 0.f);
    for (int wv = 0; wv < W; ++wv)
        for (int kc = 0; kc < kc_steps; ++kc)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < NW; ++e) {
                    const int tap = e / NBW, blk = wv * NBW + e % NBW;
                    const int co = 16 * blk + (l & 15), ci = 4 * kc + (l >> 4);
                    const float v = ci < c.cin && blk < NB ? c.w[((size_t)tap * c.cin + ci) * c.cout + co] : 0.f;
                    out[base + ((((size_t)wv * kc_steps + kc) * NCH + e / 4) * 64 + l) * 4 + (e % 4)] = v;
                }
}

int f32c_pack_weights(oth_net* net, F32Weights* fw) {
    const HostNet& hn = net->host;
    const int F = hn.filters, L = 1 + 2 * hn.blocks, W = f32c_waves(F);
    OTH_CHECK(W > 0, "fp32 cooperative trunk: no build for %d filters", F);
    std::vector<float> w;
    fw->layer_off_c.resize(L);
    for (int l = 0; l < L; ++l) {
        fw->layer_off_c[l] = (uint32_t)(w.size() / 4);
        pack_layer_c(l == 0 ? hn.stem : hn.res[l - 1], F, W, l == 0 ? 1 : F / 4, w);
    }
    return fw->wc.upload(w);
}

template <int F, int BS, int P, int W>
static int launch_f32c(oth_net* net, const F32Args& a, const uint64_t* sb, const uint64_t* ob, const uint64_t* lg,
                       int64_t n, const int32_t* n_valid, float* logp, float* v, hipStream_t stream) {
    using G = TrunkGeom<F, BS, P>;
    constexpr size_t lds = (size_t)G::WAVE_WORDS * sizeof(float);   // the planes of one position group + its head scratch
    static_assert(lds <= 160 * 1024, "LDS budget");
    if (int rc = set_max_dynamic_lds((const void*)k_trunk_f32c<F, BS, P, W>, net->device, (int)lds)) return rc;
    const unsigned grid = (unsigned)((n + P - 1) / P);
    hipLaunchKernelGGL((k_trunk_f32c<F, BS, P, W>), dim3(grid), dim3(64 * W), lds, stream, a, sb, ob, lg, n, n_valid, logp,
                       v);
    OTH_HIP(hipGetLastError());
    return OTH_OK;
}

int f32c_forward(oth_net* net, const F32Weights* fw, F32Args& a, const uint64_t* sb, const uint64_t* ob, const uint64_t* lg,
                 int64_t n, const int32_t* n_valid, float* logp, float* v, hipStream_t stream) {
    OTH_CHECK(fw->wc.get(), "fp32 cooperative trunk: weights not packed");
    a.w = fw->wc.get();
    for (int l = 0; l < a.n_layers; ++l) a.layer_off[l] = fw->layer_off_c[l];
    const int F = net->filters;
    // positions per workgroup: one on 8x8 (4 tiles of 16 cells), two on 6x6 (72 cells in 5 tiles); waves: f32c_waves
#define OTH_F32C_CASE(FF, WW)                                                                                         \
    if (F == FF && f32c_waves(FF) == WW) {                                                                            \
        if (net->board == 8) return launch_f32c<FF, 8, 1, WW>(net, a, sb, ob, lg, n, n_valid, logp, v, stream);       \
        if (net->board == 6) return launch_f32c<FF, 6, 2, WW>(net, a, sb, ob, lg, n, n_valid, logp, v, stream);       \
    }
    OTH_F32C_CASE(64, 2)
    OTH_F32C_CASE(128, 2)
    OTH_F32C_CASE(144, 3)
    OTH_F32C_CASE(160, 2)
    OTH_F32C_CASE(176, 4)
    OTH_F32C_CASE(192, 4)
    OTH_F32C_CASE(208, 4)
    OTH_F32C_CASE(224, 4)
    OTH_F32C_CASE(240, 4)
    OTH_F32C_CASE(256, 4)
#undef OTH_F32C_CASE
    set_error("fp32 cooperative trunk: unsupported filters %d / board %d", F, net->board);
    return OTH_E_UNSUPPORTED;
}

}  // namespace oth
