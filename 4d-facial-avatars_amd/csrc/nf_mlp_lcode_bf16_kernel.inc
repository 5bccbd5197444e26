// Body of the split-bf16 fused forward of the second model family (included once per translation unit with NFB_SAVE = 0 / 1
// and NFB_KERNEL_NAME set; separate translation units for the reason given in nf_mlp_bf16_kernel.inc).
// NFB_SAVE: training forward -- every layer output also goes to `saved` (sections nlc::S_*) plus the ReLU bit masks the
// split-bf16 backward chain reads (nlc::S_MASK).
// This file is the family's part: the bias-scaling list and the layer list; the rest of the body is nf_mlp_split_fwd.inc.
// NFB_SIGMA_ONLY (with NFB_RUN_LAYERS 5, NFB_SAVE 0): the density-only inference kernels -- the list ends behind fc_alpha and `raw`
// receives one float per point.
#ifndef NFB_SIGMA_ONLY
#define NFB_SIGMA_ONLY 0
#endif
#include <type_traits>
#include "nf_mlp_bf16_machinery.inc"

__global__ void __launch_bounds__(256, 1)
NFB_KERNEL_NAME(const char* __restrict__ wstream, const float* __restrict__ cond, const float* __restrict__ ro,
                const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z, int64_t n_points, int S,
                float* __restrict__ raw, float* __restrict__ saved) {
    using namespace nlc;
    // layer l of the stream <-> its bias section
#define NFB_SCALE_BIASES(bw, t)                                                      \
    bw[B_L1 + t] *= SC(0);                                                           \
    bw[B_X0 + t] *= SC(1);                                                           \
    bw[B_X1 + t] *= SC(2);                                                           \
    bw[B_X2 + t] *= SC(3);                                                           \
    bw[B_FEAT + t] *= SC(5);                                                         \
    if (t < 16) bw[B_ALPHA + t] *= SC(4);                                            \
    if (t < 128) bw[B_DIR + t] *= SC(6);
#include "nf_mlp_split_fwd.inc"
    // ReLU mask numbers: layers_xyz.0..2 -> 0..2, fc_feat -> 3, layers_dir.0 -> 4
    // ---- layer1: PE -> 256, no activation (M:609) -----------------------------------------------------------------------
    nfb_init_bias<8>(accA, bias + B_L1, h);
    NFB_LAYER(0, accA, bh, bl);
    NFB_FINISH(0, accA, 8, false, 0);
    NFB_HIDDEN_LAYER(1, accB, B_X0, true, 0, accA, S_L1);
    NFB_HIDDEN_LAYER(2, accA, B_X1, true, 1, accB, S_X0);
    NFB_HIDDEN_LAYER(3, accB, B_X2, true, 2, accA, S_X1);
    // ---- fc_alpha(x) (one tile, row 0), then feat = relu(fc_feat(x)) on the same operands -----------------------------------
    // (training: x2, the output of layers_xyz.2 = these operands, is streamed from inside fc_feat's K loop)
#pragma unroll
    for (int s = 0; s < 16; ++s) { th[s] = bh[4 + s]; tl[s] = bl[4 + s]; }
    nfb_zero(accA[0]);
    if (h == 0) accA[0][0] = bias[B_ALPHA];
    NFB_LAYER(4, accA, th, tl);
    const float sigma_raw = accA[0][0] * OUT_INV(4);
#if NFB_SIGMA_ONLY
    // density only (NFB_RUN_LAYERS = 5: the ring ends with fc_alpha's last stage)
    NFB_STORE_SIGMA();
#else
    nfb_init_bias<8>(accA, bias + B_FEAT, h);
    NFB_RUN(5, accA, th, tl, 8, accB, S_X2);
    NFB_FINISH(5, accA, 8, true, 3);
    // ---- layers_dir.0: 16 feat k-steps + dir k-step + 1 zero k-step -> 128, ReLU -----------------------------------------
    nfb_init_bias<4>(accB, bias + B_DIR, h);
#pragma unroll
    for (int s = 0; s < 16; ++s) { th[s] = bh[4 + s]; tl[s] = bl[4 + s]; }
    th[16] = dh; tl[16] = dl;
#pragma unroll
    for (int s = 17; s < nfb::KS[6]; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) { th[s][j] = (nfb_elt)0.f; tl[s][j] = (nfb_elt)0.f; }
    NFB_RUN(6, accB, th, tl, 8, accA, S_FEAT);
    NFB_FINISH(6, accB, 4, true, 4);
    // ---- fc_rgb ---------------------------------------------------------------------------------------------------------
    nfb_zero(accA[0]);
#pragma unroll
    for (int s = 0; s < 8; ++s) { th[s] = bh[4 + s]; tl[s] = bl[4 + s]; }
    NFB_RUN(7, accA, th, tl, 4, accB, S_DIR);
    NFB_STORE_RAW(7, accA, B_RGB);
#endif
}
