// Layouts of the third model family (ConditionalBlendshapePaperSmallerNeRFModel, reference nerf/models.py:266-338): packed
// weight image, per-call bias table, and -- training -- saved activations, pre-activation gradients, transposed image and
// gradient slab.  Same conventions as nf_mlp_layout.h (fragment order, PE slot order, section-major buffers).
//
// The model is the paper model without layers_xyz.5 and without the dead layers_dir.3, and with the expression appended to
// layers_dir.0's input: [feat 256 | PE4(dir) 24 | expr/3 76] -> 128.  The expression is constant per call, so those 76 columns
// fold into layers_dir.0's bias beside the 16 near / far columns (Quirk Q1).
#pragma once
#include "nf_mlp_layout.h"

namespace nsm {
// ---- MFMA layers -------------------------------------------------------------------------------
//                       K chunks                        N tiles
// L0  (layers_xyz.0)    4  (PE slots)                   16
// L1,L2,L4,FEAT         16 (hidden)                     16
// L3  (layers_xyz.3)    4 (PE) + 16 (hidden)            16
// D0  (layers_dir.0)    16 (feat) + 1 (dir slots)       8 + 1 (tile 8, row 0 = fc_alpha)
// D1,D2                 8                               8
// RGB (fc_rgb)          8                               1 (rows 0..2)
constexpr int FRAG = 256;
constexpr int OFF_L0 = 0;
constexpr int OFF_L1 = OFF_L0 + 4 * 16 * FRAG;
constexpr int OFF_L2 = OFF_L1 + 16 * 16 * FRAG;
constexpr int OFF_L3 = OFF_L2 + 16 * 16 * FRAG;
constexpr int OFF_L4 = OFF_L3 + 20 * 16 * FRAG;
constexpr int OFF_FEAT = OFF_L4 + 16 * 16 * FRAG;
constexpr int OFF_D0 = OFF_FEAT + 16 * 16 * FRAG;
constexpr int OFF_D1 = OFF_D0 + 17 * 9 * FRAG;
constexpr int OFF_D2 = OFF_D1 + 8 * 8 * FRAG;
constexpr int OFF_RGB = OFF_D2 + 8 * 8 * FRAG;
constexpr int FRAG_END = OFF_RGB + 8 * 1 * FRAG;
// ---- conditioning matrices (row-major) -----------------------------------------------------------
constexpr int NCOND = 108;                      // 76 expression + 32 latent columns
constexpr int NEXPR = 76;
constexpr int OFF_WC0 = FRAG_END;               // [256][108] = layers_xyz.0.weight[:, 63:171]
constexpr int OFF_WC3 = OFF_WC0 + 256 * NCOND;  // [256][108] = layers_xyz.3.weight[:, 63:171]
constexpr int OFF_WCD = OFF_WC3 + 256 * NCOND;  // [128][16]  = layers_dir.0.weight[:, 256+6f+3sc+{1,2}], col = 4f+2sc+(comp-1)
constexpr int OFF_WCE = OFF_WCD + 128 * 16;     // [128][76]  = layers_dir.0.weight[:, 280:356]
constexpr int OFF_BIAS = OFF_WCE + 128 * NEXPR; // un-folded bias table, same layout as `cond`
// ---- bias table / cond layout ----------------------------------------------------------------------
constexpr int B_L0 = 0, B_L1 = 256, B_L2 = 512, B_L3 = 768, B_L4 = 1024, B_FEAT = 1280;
constexpr int B_D0 = 1536;                      // 128 + 16 (alpha tile: [fc_alpha.bias, 0 x 15])
constexpr int B_D1 = B_D0 + 144, B_D2 = B_D1 + 128, B_RGB = B_D2 + 128;   // rgb tile: [b_r, b_g, b_b, 0 x 13]
constexpr int BIAS_FLOATS = B_RGB + 16;         // 1952
constexpr int B_CVEC = BIAS_FLOATS;             // cond only: [expr*1/3 (76) | latent (32)] as the kernels used it
constexpr int B_DVEC = B_CVEC + NCOND;          // cond only: PE4 of (near, far): index 4f + 2sc + (0: near, 1: far)
constexpr int COND_FLOATS = B_DVEC + 16;        // 2076
// layers_dir.0 for PRE-ENCODED inputs (model.forward(x87, ...)): 16 feat chunks + 2 chunks holding the 24 reference direction
// columns 256..279 in reference order (slot 256 + s <-> column 256 + s, s < 24), 9 tiles as OFF_D0 (cf. nfl::OFF_D0E)
constexpr int OFF_D0E = OFF_BIAS + BIAS_FLOATS;
constexpr int PACKED = OFF_D0E + 18 * 9 * FRAG;
constexpr int NPARAMS = 22;   // layers_xyz.0..4, fc_feat, fc_alpha, layers_dir.0..2, fc_rgb (weight, bias each): state_dict order

// ---- training: activations saved by the forward, floats per point (section X of an n-point buffer starts at X * n) ----
constexpr int S_PE = 0;                                              // 64, PE slot order
constexpr int S_H0 = 64, S_H1 = 320, S_H2 = 576, S_H3 = 832, S_H4 = 1088;   // 256 each, post-ReLU
constexpr int S_FEAT = 1344;                                         // 256, fc_feat output
constexpr int S_D0 = 1600, S_D1 = 1728, S_D2 = 1856;                 // 128 each, post-ReLU
constexpr int S_DIRF = 1984;                                         // 16, dir slot order (sin, cos, 0, 0)(rd_z 2^g)
constexpr int S_MASK = 2000;                                         // ReLU bit masks, 8 layers (h0..h4, layers_dir.0..2): nf_mask_ptr
constexpr int N_RELU = 8;
constexpr int SAVED_PER_POINT = S_MASK + N_RELU * 8;
// ---- pre-activation gradients written by the backward chain ------------------------------------------------------
constexpr int Z_L0 = 0, Z_L1 = 256, Z_L2 = 512, Z_L3 = 768, Z_L4 = 1024, Z_FEAT = 1280;
constexpr int Z_D0 = 1536, Z_D1 = 1664, Z_D2 = 1792;
constexpr int DZ_PER_POINT = 1920;
// ---- transposed image for the backward chain: block (ni, no), lane (g, i), r -> W[16 ni + 4 g + r][col0 + 16 no + i] ----
constexpr int OFFT_RGB = 0;                               // 1 chunk (3 rows) x 8 tiles
constexpr int OFFT_D2 = OFFT_RGB + 1 * 8 * FRAG;
constexpr int OFFT_D1 = OFFT_D2 + 8 * 8 * FRAG;
constexpr int OFFT_D0 = OFFT_D1 + 8 * 8 * FRAG;           // layers_dir.0[:, :256]: 8 chunks x 16 tiles, then chunk 8: slot 0 = fc_alpha.weight
constexpr int OFFT_FEAT = OFFT_D0 + 9 * 16 * FRAG;
constexpr int OFFT_L4 = OFFT_FEAT + 16 * 16 * FRAG;
constexpr int OFFT_L3 = OFFT_L4 + 16 * 16 * FRAG;         // layers_xyz.3[:, 171:427]
constexpr int OFFT_L2 = OFFT_L3 + 16 * 16 * FRAG;
constexpr int OFFT_L1 = OFFT_L2 + 16 * 16 * FRAG;
constexpr int PACKED_T = OFFT_L1 + 16 * 16 * FRAG;
// ---- gradient slab (per point slice), then the flat gradient vector in state_dict order + d latent -------------
constexpr int G_L0 = 0;                          // [256][64]   (PE slot order)
constexpr int G_L1 = G_L0 + 256 * 64;            // [256][256]
constexpr int G_L2 = G_L1 + 65536;
constexpr int G_L3A = G_L2 + 65536;              // [256][64]   (PE slot order)
constexpr int G_L3B = G_L3A + 256 * 64;          // [256][256]  (hidden part, reference columns 171..426)
constexpr int G_L4 = G_L3B + 65536;
constexpr int G_FEAT = G_L4 + 65536;
constexpr int G_D0A = G_FEAT + 65536;            // [128][256]
constexpr int G_D0B = G_D0A + 128 * 256;         // [128][16]   (dir slot order)
constexpr int G_D1 = G_D0B + 128 * 16;           // [128][128]
constexpr int G_D2 = G_D1 + 128 * 128;
constexpr int G_RGB = G_D2 + 128 * 128;          // [16][128]   rows 0..2 = fc_rgb.weight grad
constexpr int G_ALPHA = G_RGB + 16 * 128;        // [16][256]   row 3 (the d sigma column of d_raw) = fc_alpha.weight grad
constexpr int CS_L0 = G_ALPHA + 16 * 256;        // column sums of dZ = bias grads: 6 x 256 (layers_xyz.0..4, fc_feat)
constexpr int CS_D0 = CS_L0 + 6 * 256;           // 3 x 128
constexpr int CS_RGB = CS_D0 + 3 * 128;          // 16: [d b_r, d b_g, d b_b, d b_alpha, 0...]
constexpr int SLAB_FLOATS = CS_RGB + 16;
constexpr int GRAD_PARAM_FLOATS = 496132;        // the 22 tensors, state_dict order, flattened
constexpr int GRAD_FLOATS = GRAD_PARAM_FLOATS + 32;   // + d latent
}  // namespace nsm
