// Body of the split-bf16 fused forward (included once per translation unit with NFB_SAVE = 0 / 1 and NFB_KERNEL_NAME set):
// the inference and the training (activation-saving) instantiations live in SEPARATE translation units on purpose --
// co-compiled instantiations of this kernel perturb each other's register allocation / schedule by up to 20 %.
// NFB_SAVE: training forward -- the layer outputs also go to `saved` (sections nfl::S_*) as the weight-gradient kernel's fragment
// streams, plus the ReLU bit masks the split backward chain reads (nfl::S_MASK).
// This file is the paper model's part: the bias-scaling list and the layer list; the rest of the body is nf_mlp_split_fwd.inc.
// NFB_SIGMA_ONLY (with NFB_RUN_LAYERS 8, NFB_SAVE 0): the density-only inference kernels -- the list ends behind layers_dir.0, whose
// tile 4 is fc_alpha, and `raw` receives one float per point.
#ifndef NFB_SIGMA_ONLY
#define NFB_SIGMA_ONLY 0
#endif
#include <type_traits>
#include "nf_mlp_bf16_machinery.inc"

__global__ void __launch_bounds__(256, 1)
NFB_KERNEL_NAME(const char* __restrict__ wstream, const float* __restrict__ cond, const float* __restrict__ ro,
                     const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z,
                     int64_t n_points, int S, float* __restrict__ raw, float* __restrict__ saved) {
    using namespace nfl;
    // stream layers 0..6 <-> the seven 256-float bias sections B_L0 .. B_FEAT, 7..9 <-> layers_dir.0 (+ fc_alpha's bias), .1, .2
#define NFB_SCALE_BIASES(bw, t)                                                      \
    _Pragma("unroll") for (int l = 0; l < 7; ++l) bw[256 * l + t] *= SC(l);          \
    if (t < 144) bw[B_D0 + t] *= SC(7);                                              \
    if (t < 128) { bw[B_D1 + t] *= SC(8); bw[B_D2 + t] *= SC(9); }
#include "nf_mlp_split_fwd.inc"
    // ---- layers_xyz.0 : PE -> 256 --------------------------------------------------------------------------
    nfb_init_bias<8>(accA, bias + B_L0, h);
    NFB_LAYER(0, accA, bh, bl);
    NFB_FINISH(0, accA, 8, true, nfb_mask_index(S_H0));
    NFB_HIDDEN_LAYER(1, accB, B_L1, true, nfb_mask_index(S_H1), accA, S_H0);
    NFB_HIDDEN_LAYER(2, accA, B_L2, true, nfb_mask_index(S_H2), accB, S_H1);
    // ---- layers_xyz.3 : [PE | h] (20 k-steps: operands 0..19 as they sit) ------------------------------------------
    nfb_init_bias<8>(accB, bias + B_L3, h);
    NFB_RUN(3, accB, bh, bl, 8, accA, S_H2);
    NFB_FINISH(3, accB, 8, true, nfb_mask_index(S_H3));
    NFB_HIDDEN_LAYER(4, accA, B_L4, true, nfb_mask_index(S_H4), accB, S_H3);
    NFB_HIDDEN_LAYER(5, accB, B_L5, true, nfb_mask_index(S_H5), accA, S_H4);
    NFB_HIDDEN_LAYER(6, accA, B_FEAT, false, nfb_mask_index(S_FEAT), accB, S_H5);
    // ---- layers_dir.0 (+ fc_alpha as tile 4): 16 feat k-steps + dir k-step + 1 zero k-step ------------------------------
    nfb_init_bias<4>(accB, bias + B_D0, h);
    nfb_zero(accB[4]);
    if (h == 0) accB[4][0] = bias[B_D0 + 128];
#pragma unroll
    for (int s = 0; s < 16; ++s) { th[s] = bh[4 + s]; tl[s] = bl[4 + s]; }
    th[16] = dh; tl[16] = dl;
#pragma unroll
    for (int s = 17; s < nfb::KS[7]; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) { th[s][j] = (nfb_elt)0.f; tl[s][j] = (nfb_elt)0.f; }
    NFB_RUN(7, accB, th, tl, 8, accA, S_FEAT);
    const float sigma_raw = accB[4][0] * OUT_INV(7);
#if NFB_SIGMA_ONLY
    // density only (NFB_RUN_LAYERS = 8: the ring ends with this layer's last stage)
    NFB_STORE_SIGMA();
#else
    NFB_FINISH(7, accB, 4, true, nfb_mask_index(S_D0));
    // ---- layers_dir.1, .2 ----------------------------------------------------------------------------------------------
    nfb_init_bias<4>(accA, bias + B_D1, h);
#pragma unroll
    for (int s = 0; s < 8; ++s) { th[s] = bh[4 + s]; tl[s] = bl[4 + s]; }
    NFB_RUN(8, accA, th, tl, 4, accB, S_D0);
    NFB_FINISH(8, accA, 4, true, nfb_mask_index(S_D1));
    nfb_init_bias<4>(accB, bias + B_D2, h);
#pragma unroll
    for (int s = 0; s < 8; ++s) { th[s] = bh[4 + s]; tl[s] = bl[4 + s]; }
    NFB_RUN(9, accB, th, tl, 4, accA, S_D1);
    NFB_FINISH(9, accB, 4, true, nfb_mask_index(S_D2));
    // ---- fc_rgb -----------------------------------------------------------------------------------------------------------
    nfb_zero(accA[0]);
#pragma unroll
    for (int s = 0; s < 8; ++s) { th[s] = bh[4 + s]; tl[s] = bl[4 + s]; }
    NFB_RUN(10, accA, th, tl, 4, accB, S_D2);
    NFB_STORE_RAW(10, accA, B_RGB);
#endif
}
