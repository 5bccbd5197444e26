// The exact-f32 network of the second model family, written once: ConditionalBlendshapeLearnableCodeNeRFModel (layouts nlc::, kernels
// in nf_mlp_lcode.hip / nf_mlp_lcode_sigma.hip / nf_mlp_lcode_bwd.hip) and the two blendshape classes that per point ARE that network
// (nf_mlp_bshape.h).  This header holds the forward half -- the trunk's bias table (the body of every condition kernel of the three
// classes) and the inference layer stream; the __global__ kernels keep their names in their translation units and wrap these.
// Backward: nf_mlp_lcode_net_bwd.h.  What both network shapes share is in nf_mlp_net_common.h.
#pragma once
#include <vector>
#include "nf_mlp_net_common.h"
#include "nf_mlp_lcode_layout.h"
#include "nf_pack.h"

// what the shared stream text (nf_mlp_net_common.h) reads of a family's layout
struct NfLcodeNet {
    static constexpr int S_MASK = nlc::S_MASK, PACKED_T = nlc::PACKED_T, OFFT_RGB = nlc::OFFT_RGB;
};

// ---- what the family's forward translation units provide to the classes that run on it -----------------------------------
void nf_lcode_build_table(std::vector<uint32_t>& t, const NfLcodeGeom& ge);           // exact-f32 image (nf_mlp_lcode.hip)
void nf_lcode_build_table_bf16(std::vector<uint32_t>& t, const NfLcodeGeom& ge);      // (hi, lo) stream (nf_mlp_lcode_bf16.hip)
float nf_lcode_f16_stream_layers(int* pair_off);                                      // 8 + 1 offsets; returns the activation pre-scale
// k_lcode_mlp_fwd_encoded on a bias table that is already filled
int nf_lcode_launch_fwd_encoded(const float* packed, const float* cond, const float* x87, int64_t n_points, float* out, nf_stream_t stream);

// =================================================================================================
// condition: per-call bias table of the trunk
//   cond[L1]  = b1  + layer1.weight[:, 63:63 + N_COND] . cvec      (the class's folded vector: [expr/3 | latent], expr/3, or e3)
//   cond[DIR] = bd0 + Wd0[:, 256 + 6f + 3sc + {1,2}] . {sin,cos}({near,far} 2^f)            (not ENCODED)
//   every other entry is the plain bias; cvec and dvec follow the table for the backward.
// =================================================================================================
// entry k of the (near, far) direction features folded into layers_dir.0's bias
__device__ __forceinline__ float nf_lcode_dvec(int k, float near_z, float far_z) {
    const int f = k >> 2, sc = (k >> 1) & 1, comp = k & 1;
    const float a = nf_mul(comp ? far_z : near_z, exp2f((float)f));
    return sc ? cosf(a) : sinf(a);
}

// The table from cvec[108] (LDS; entries past N_COND are zero) and dvec[16], after the barrier that publishes them.  ENCODED: the
// table of <prefix>_forward_encoded (the direction columns arrive with x: no fold, dvec is not read and 0 is stored for it).
// first / stride: the thread's grid-stride loop, formed in the calling kernel (where the compiler folds the block size of a uniform
// launch into one scalar load; in a device function it selects between full and remainder size with a vector load).
template <int N_COND, bool ENCODED>
__device__ __forceinline__ void nf_lcode_bias_table(const float* __restrict__ packed, const float* cvec, const float* dvec,
                                                    float* __restrict__ cond, int first = blockIdx.x * blockDim.x + threadIdx.x,
                                                    int stride = gridDim.x * blockDim.x) {
    using namespace nlc;
    const float* bias = packed + OFF_BIAS;
    for (int i = first; i < COND_FLOATS; i += stride) {
        if (i >= B_CVEC) { cond[i] = i < B_DVEC ? cvec[i - B_CVEC] : (ENCODED ? 0.0f : dvec[i - B_DVEC]); continue; }
        float v = bias[i];
        if (i < B_X0) {
            const float* w = packed + OFF_WC1 + i * 108;
            float s = 0.0f;
            for (int k = 0; k < N_COND; ++k) s = fmaf(w[k], cvec[k], s);
            v += s;
        } else if (!ENCODED && i >= B_DIR && i < B_DIR + 128) {
            const float* w = packed + OFF_WCD + (i - B_DIR) * 16;
            float s = 0.0f;
            for (int k = 0; k < 16; ++k) s = fmaf(w[k], dvec[k], s);
            v += s;
        }
        cond[i] = v;
    }
}

// =================================================================================================
// forward
//   x = layer1([PE | folded vector])  (no activation);  3 x relu(layers_xyz.i(x));  sigma = fc_alpha(x);  feat = relu(fc_feat(x));
//   relu(layers_dir.0([feat | dir])) -> rgb = fc_rgb
// =================================================================================================
// The network from layer1 to fc_rgb on the inference schedule (nf_mlp_stream.h; the form of nf_paper_net_body), shared by the
// ray-input kernel, the pre-encoded one and the density-only one.  layers_xyz.2's output feeds fc_alpha AND fc_feat: fc_alpha's tail
// stores nothing (NO_ST = 0), so fc_feat reads the same slab again.  NDIR register chunks of direction slots follow layers_dir.0's
// 16 feat chunks (1: (sin, cos)(rd_z 2^g), weights OFF_DIR, prefetched a layer ahead; 2: the 24 reference columns, weights OFF_DIRE).
// Leaves rgb_raw in acc[t][0].xyz and sigma_raw in sigma_raw[t].
// SIGMA: the density-only forward ends with fc_alpha -- its last chunk with nothing fetched behind it (same MFMAs, same order as
// nf_tail issues); leaves sigma_raw[t] alone.
template <int NT, int NDIR, bool SIGMA = false>
__device__ __forceinline__ void nf_lcode_net_body(f32x4 (&acc)[NT][16], float (&sigma_raw)[NT], const f32x4 (&pe)[NT][4],
                                                  const f32x4 (&dirf)[NT][NDIR], const NfW& Wi, const NfW& Ci, f32x4* act4, int lane) {
    using namespace nlc;
    constexpr unsigned DIR = (NDIR == 1 ? OFF_DIR : OFF_DIRE) / 4;
    NfStream<NT> st;
    f32x4 bj[NT];
    NF_NET_PE_LAYER(B_L1, OFF_L1, OFF_X0, B_X0);                                    // layer1: no activation (M:609)
    nf_seg_lds<NT, 16, true, false>(acc, st, Wi, OFF_X0 / 4, 16, act4, lane);       // reads layer1's output as stored
    nf_pending_b<NT, false>(bj, st);
    nf_tail<NT, 16, 16, 16, 1>(acc, st.wb, bj, st, Wi, OFF_X1 / 4, Ci, B_X1, act4, lane);
    nf_seg_lds<NT, 16, true, true>(acc, st, Wi, OFF_X1 / 4, 16, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 16, 16, 16, 1>(acc, st.wb, bj, st, Wi, OFF_X2 / 4, Ci, B_X2, act4, lane);
    nf_seg_lds<NT, 16, true, true>(acc, st, Wi, OFF_X2 / 4, 16, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 16, 16, 1, 1>(acc, st.wb, bj, st, Wi, OFF_ALPHA / 4, Ci, B_ALPHA, act4, lane);
    nf_seg_lds<NT, 1, true, true>(acc, st, Wi, OFF_ALPHA / 4, 16, act4, lane);      // fc_alpha(x)
    nf_pending_b<NT, true>(bj, st);
    if constexpr (SIGMA) {
        nf_chunk<NT, 1, false>(acc, st.wb, bj, st.bias);
#pragma unroll
        for (int t = 0; t < NT; ++t) sigma_raw[t] = acc[t][0].x;
        return;
    }
    nf_tail<NT, 1, 0, 16, 1>(acc, st.wb, bj, st, Wi, OFF_FEAT / 4, Ci, B_FEAT, act4, lane);
#pragma unroll
    for (int t = 0; t < NT; ++t) sigma_raw[t] = acc[t][0].x;
    nf_seg_lds<NT, 16, true, true>(acc, st, Wi, OFF_FEAT / 4, 16, act4, lane);      // feat = relu(fc_feat(x)): the ReLU is the reader's
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 16, 16, 8, 1>(acc, st.wb, bj, st, Wi, DIR, Ci, B_DIR, act4, lane);
    {
        f32x4 wd[16];
        nf_load_w16<8>(wd, Wi, DIR + 16 * 8 * 64, lane);                            // the first direction chunk's weights, a layer ahead
        nf_seg_lds<NT, 8, true, true>(acc, st, Wi, DIR, 16, act4, lane);            // relu(layers_dir.0([feat | dir]))
        nf_pending_b<NT, true>(bj, st);
        nf_chunk<NT, 8, false>(acc, st.wb, bj, st.bias);
        if (NDIR == 2) {
            nf_load_w16<8>(st.wb, Wi, DIR + 17 * 8 * 64, lane);
#pragma unroll
            for (int t = 0; t < NT; ++t) bj[t] = dirf[t][0];
            nf_chunk<NT, 8, false>(acc, wd, bj, st.bias);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) bj[t] = dirf[t][NDIR - 1];
        if constexpr (NDIR == 2) nf_tail<NT, 8, 8, 1, 1>(acc, st.wb, bj, st, Wi, OFF_RGB / 4, Ci, B_RGB, act4, lane);
        else nf_tail<NT, 8, 8, 1, 1>(acc, wd, bj, st, Wi, OFF_RGB / 4, Ci, B_RGB, act4, lane);
    }
    nf_seg_lds<NT, 1, true, true>(acc, st, Wi, OFF_RGB / 4, 8, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_chunk<NT, 1, false>(acc, st.wb, bj, st.bias);
}
