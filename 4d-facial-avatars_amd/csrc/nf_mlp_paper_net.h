// The exact-f32 "paper-shaped" network, written once for its two families: ConditionalBlendshapePaperNeRFModel (layouts nfl::,
// kernels in nf_mlp.hip / nf_mlp_encoded.hip / nf_mlp_bwd.hip) and ConditionalBlendshapePaperSmallerNeRFModel (layouts nsm::,
// nf_mlp_smaller.hip / nf_mlp_smaller_bwd.hip).  Both are the same hand-scheduled layer stream (nf_mlp_stream.h); a family is a traits
// struct over its layout namespace plus two discriminators:
//   HAS_L5   the 256-wide hidden layer layers_xyz.5 exists (and with it tensor ids, sections and ReLU layers behind layers_xyz.4 shift)
//   D0_EXPR  the 76 expression columns enter layers_dir.0 a second time (folded into its bias; its weight is [128][D0_COLS])
// This header holds the forward half: gather table, bias-table (condition) kernel body, the inference and the saving layer stream.
// The __global__ kernels keep their names in their translation units and wrap these.  Backward: nf_mlp_paper_net_bwd.h.  Input
// fragments, the `raw` store and the stream text shared with the second family's network: nf_mlp_net_common.h.
#pragma once
#include "nf_mlp_net_common.h"
#include "nf_mlp_smaller_layout.h"
#include "nf_pack.h"

// what nfl:: and nsm:: name alike (values differ)
#define NF_NET_COMMON(F)                                                                                                              \
    F(FRAG) F(NCOND) F(OFF_L0) F(OFF_L1) F(OFF_L2) F(OFF_L3) F(OFF_L4) F(OFF_FEAT) F(OFF_D0) F(OFF_D0E) F(OFF_D1) F(OFF_D2) F(OFF_RGB) \
    F(OFF_WC0) F(OFF_WC3) F(OFF_WCD) F(OFF_BIAS) F(B_L0) F(B_L1) F(B_L2) F(B_L3) F(B_L4) F(B_FEAT) F(B_D0) F(B_D1) F(B_D2) F(B_RGB)     \
    F(B_CVEC) F(B_DVEC) F(COND_FLOATS) F(S_PE) F(S_H0) F(S_H1) F(S_H2) F(S_H3) F(S_H4) F(S_FEAT) F(S_D0) F(S_D1) F(S_D2) F(S_DIRF)     \
    F(S_MASK) F(SAVED_PER_POINT) F(Z_L0) F(Z_L1) F(Z_L2) F(Z_L3) F(Z_L4) F(Z_FEAT) F(Z_D0) F(Z_D1) F(Z_D2) F(DZ_PER_POINT)             \
    F(OFFT_RGB) F(OFFT_D2) F(OFFT_D1) F(OFFT_D0) F(OFFT_FEAT) F(OFFT_L4) F(OFFT_L3) F(OFFT_L2) F(OFFT_L1)                              \
    F(G_L0) F(G_L1) F(G_L2) F(G_L3A) F(G_L3B) F(G_L4) F(G_FEAT) F(G_D0A) F(G_D0B) F(G_D1) F(G_D2) F(G_RGB) F(G_ALPHA)                  \
    F(CS_L0) F(CS_D0) F(CS_RGB) F(SLAB_FLOATS) F(GRAD_PARAM_FLOATS) F(GRAD_FLOATS)

struct NfPaperNet {
#define NF_NET_COPY(X) static constexpr int X = nfl::X;
    NF_NET_COMMON(NF_NET_COPY)
    NF_NET_COPY(OFF_L5) NF_NET_COPY(B_L5) NF_NET_COPY(S_H5) NF_NET_COPY(Z_L5) NF_NET_COPY(OFFT_L5) NF_NET_COPY(G_L5)
#undef NF_NET_COPY
    static constexpr bool HAS_L5 = true, D0_EXPR = false;
    static constexpr int PACKED = nfl::PACKED_FLOATS, PACKED_T = nfl::PACKED_T_FLOATS, NPARAMS = NF_PAPER_NUM_PARAMS;
    static constexpr int N_RELU = (nfl::SAVED_PER_POINT - nfl::S_MASK) / 8;
    static constexpr int D0_COLS = 280;                       // layers_dir.0.weight: [feat 256 | PE4(dir) 24]
    static constexpr int MODEL = 0;                           // k_dw_gemm_lds<M> / k_grad_reduce<M> instantiation
};

struct NfSmallerNet {
#define NF_NET_COPY(X) static constexpr int X = nsm::X;
    NF_NET_COMMON(NF_NET_COPY)
    NF_NET_COPY(OFF_WCE) NF_NET_COPY(NEXPR) NF_NET_COPY(PACKED) NF_NET_COPY(PACKED_T) NF_NET_COPY(NPARAMS) NF_NET_COPY(N_RELU)
#undef NF_NET_COPY
    static constexpr bool HAS_L5 = false, D0_EXPR = true;
    static constexpr int D0_COLS = 280 + nsm::NEXPR;          // [feat 256 | PE4(dir) 24 | expr/3 76]
    static constexpr int MODEL = 2;
};
#undef NF_NET_COMMON

// 256-wide ReLU layers in front of fc_feat; their biases are the first N rows of the bias table, their masks ReLU layers 0 .. N - 1,
// and layers_dir.0..2 are ReLU layers N .. N + 2
template <class Net> constexpr int nf_net_n_xyz = Net::HAS_L5 ? 6 : 5;

// Tensor roles = the paper model's state_dict ids; a family without layers_xyz.5 (and without the dead layers_dir.3, ids 22 / 23)
// numbers the tensors behind them lower.  fc_rgb is the last pair of every family.
enum { NF_R_XYZ0_W = 0, NF_R_XYZ3_W = 6, NF_R_L5_W = 10, NF_R_FEAT_W = 12, NF_R_FEAT_B = 13, NF_R_ALPHA_W = 14, NF_R_ALPHA_B = 15,
       NF_R_DIR0_W = 16, NF_R_DIR0_B = 17, NF_R_DIR1_W = 18, NF_R_DIR2_W = 20, NF_R_RGB_W = 24, NF_R_RGB_B = 25 };
template <class Net>
__host__ __device__ constexpr int nf_net_id(int role) {
    return role >= NF_R_RGB_W ? Net::NPARAMS - 2 + (role - NF_R_RGB_W) : (role >= NF_R_FEAT_W && !Net::HAS_L5 ? role - 2 : role);
}
template <class Net>
__host__ __device__ constexpr int nf_net_role(int id) {
    return id >= Net::NPARAMS - 2 ? NF_R_RGB_W + (id - (Net::NPARAMS - 2)) : (id >= NF_R_L5_W && !Net::HAS_L5 ? id + 2 : id);
}

// =================================================================================================
// pack: gather the nn.Parameter storages into the fragment-ordered image
// =================================================================================================
template <class Net>
static void nf_paper_net_table(std::vector<uint32_t>& t) {
    constexpr int NX = nf_net_n_xyz<Net>;
    auto id = [](int role) { return nf_net_id<Net>(role); };
    t.assign(Net::PACKED, NF_ZERO_CODE);
    // col_of(slot) -> reference column of `tensor` (or -1 = zero); rows >= n_out are zero, except that `alpha_row` (if >= 0) is
    // served from fc_alpha.weight (fc_alpha reads feat only: slots 0..255)
    auto fill = [&](int off, int nk, int no_tiles, int tensor, int n_out, int n_cols, auto col_of, int alpha_row = -1) {
        nf_fill_frag(t, off, nk, no_tiles, [&](int slot, int n) {
            if (n < n_out) {
                const int col = col_of(slot);
                return col >= 0 ? nf_code(tensor, n, col, n_cols) : NF_ZERO_CODE;
            }
            return n == alpha_row && slot < 256 ? nf_code(id(NF_R_ALPHA_W), 0, slot, 256) : NF_ZERO_CODE;
        });
    };
    auto ident = [](int s) { return s; };
    fill(Net::OFF_L0, 4, 16, NF_R_XYZ0_W, 256, 171, [](int s) { return nfl::pe_slot_to_col(s); });
    fill(Net::OFF_L1, 16, 16, 2, 256, 256, ident);
    fill(Net::OFF_L2, 16, 16, 4, 256, 256, ident);
    fill(Net::OFF_L3, 20, 16, NF_R_XYZ3_W, 256, 427, [](int s) { return s < 64 ? nfl::pe_slot_to_col(s) : 171 + (s - 64); });
    fill(Net::OFF_L4, 16, 16, 8, 256, 256, ident);
    if constexpr (Net::HAS_L5) fill(Net::OFF_L5, 16, 16, NF_R_L5_W, 256, 256, ident);
    fill(Net::OFF_FEAT, 16, 16, id(NF_R_FEAT_W), 256, 256, ident);
    // layers_dir.0: slots 0..255 = feat; chunk 16: lane group g holds (sin, cos)(rd_z * 2^g) at r = 0, 1
    fill(Net::OFF_D0, 17, 9, id(NF_R_DIR0_W), 128, Net::D0_COLS,
         [](int s) {
             if (s < 256) return s;
             const int g = ((s - 256) >> 2) & 3, r = (s - 256) & 3;
             return r < 2 ? 256 + 6 * g + 3 * r : -1;
         },
         /*alpha_row=*/128);
    fill(Net::OFF_D0E, 18, 9, id(NF_R_DIR0_W), 128, Net::D0_COLS, [](int s) { return s < 280 ? s : -1; }, /*alpha_row=*/128);
    fill(Net::OFF_D1, 8, 8, id(NF_R_DIR1_W), 128, 128, ident);
    fill(Net::OFF_D2, 8, 8, id(NF_R_DIR2_W), 128, 128, ident);
    fill(Net::OFF_RGB, 8, 1, id(NF_R_RGB_W), 3, 128, ident);
    for (int n = 0; n < 256; ++n)
        for (int k = 0; k < Net::NCOND; ++k) {
            t[Net::OFF_WC0 + n * Net::NCOND + k] = nf_code(NF_R_XYZ0_W, n, 63 + k, 171);
            t[Net::OFF_WC3 + n * Net::NCOND + k] = nf_code(NF_R_XYZ3_W, n, 63 + k, 427);
        }
    for (int n = 0; n < 128; ++n) {
        for (int f = 0; f < 4; ++f)
            for (int sc = 0; sc < 2; ++sc)
                for (int comp = 1; comp < 3; ++comp)
                    t[Net::OFF_WCD + n * 16 + 4 * f + 2 * sc + (comp - 1)] = nf_code(id(NF_R_DIR0_W), n, 256 + 6 * f + 3 * sc + comp, Net::D0_COLS);
        if constexpr (Net::D0_EXPR)
            for (int k = 0; k < Net::NEXPR; ++k) t[Net::OFF_WCE + n * Net::NEXPR + k] = nf_code(id(NF_R_DIR0_W), n, 280 + k, Net::D0_COLS);
    }
    for (int n = 0; n < 256; ++n) {
        for (int l = 0; l < NX; ++l) t[Net::OFF_BIAS + 256 * l + n] = nf_code(2 * l + 1, 0, n, 256);        // B_L0 .. : layers_xyz.l.bias
        t[Net::OFF_BIAS + Net::B_FEAT + n] = nf_code(id(NF_R_FEAT_B), 0, n, 256);
    }
    for (int n = 0; n < 128; ++n) {
        t[Net::OFF_BIAS + Net::B_D0 + n] = nf_code(id(NF_R_DIR0_B), 0, n, 128);
        t[Net::OFF_BIAS + Net::B_D1 + n] = nf_code(id(NF_R_DIR1_W) + 1, 0, n, 128);
        t[Net::OFF_BIAS + Net::B_D2 + n] = nf_code(id(NF_R_DIR2_W) + 1, 0, n, 128);
    }
    t[Net::OFF_BIAS + Net::B_D0 + 128] = nf_code(id(NF_R_ALPHA_B), 0, 0, 1);
    for (int n = 0; n < 3; ++n) t[Net::OFF_BIAS + Net::B_RGB + n] = nf_code(id(NF_R_RGB_B), 0, n, 3);
}

// + one point tile of mask words per ReLU layer: the exact-f32 masks are kept per 16-point tile, ceil(n / 16) of them per layer
// (sized for the split training layout too: its sections are n_points rounded up to 32 points long, nf_mlp_bf16_machinery.inc)
template <class Net>
static inline size_t nf_paper_net_saved_floats(int64_t n_points) {
    return (size_t)Net::SAVED_PER_POINT * (size_t)((n_points + 31) & ~(int64_t)31) + Net::N_RELU * 128;
}

// =================================================================================================
// condition: per-call bias table
//   cond[L0]  = b0  + W0[:, 63:139] (expr*1/3) + W0[:, 139:171] latent
//   cond[L3]  = b3  + W3[:, 63:171] [expr/3 ; latent]
//   cond[D0]  = bd0 + Wd0[:, 256 + 6f + 3sc + {1,2}] . {sin,cos}({near,far} 2^f)         (Quirk Q1; DIRS only)
//                   + Wd0[:, 280:356] (expr*1/3)                                         (D0_EXPR only)
//   every other entry is the plain bias.  DIRS = false (pre-encoded inputs): the direction columns arrive with x, no Q1 fold.
// =================================================================================================
template <class Net, bool DIRS>
__device__ __forceinline__ void nf_paper_net_condition(const float* __restrict__ packed, const float* __restrict__ expr,
                                                       const float* __restrict__ latent, float near_z, float far_z, float* __restrict__ cond) {
    __shared__ float cvec[Net::NCOND];
    __shared__ float dvec[16];
    const int tid = threadIdx.x;
    if (tid < 76) cvec[tid] = nf_div(nf_mul(expr[tid], 1.0f), 3.0f);        // (expr * 1) / 3, a true division
    else if (tid < Net::NCOND) cvec[tid] = latent[tid - 76];
    if (tid >= 128 && tid < 144) {
        const int k = tid - 128, f = k >> 2, sc = (k >> 1) & 1, comp = k & 1;
        const float a = nf_mul(comp ? far_z : near_z, exp2f((float)f));
        dvec[k] = DIRS ? (sc ? cosf(a) : sinf(a)) : 0.0f;
    }
    __syncthreads();
    const float* bias = packed + Net::OFF_BIAS;
    for (int i = blockIdx.x * blockDim.x + tid; i < Net::COND_FLOATS; i += gridDim.x * blockDim.x) {
        if (i >= Net::B_CVEC) { cond[i] = i < Net::B_DVEC ? cvec[i - Net::B_CVEC] : dvec[i - Net::B_DVEC]; continue; }
        float v = bias[i];
        if (i < Net::B_L1 || (i >= Net::B_L3 && i < Net::B_L4)) {
            const int n = i < Net::B_L1 ? i : i - Net::B_L3;
            const float* w = packed + (i < Net::B_L1 ? Net::OFF_WC0 : Net::OFF_WC3) + n * Net::NCOND;
            float s = 0.0f;
            for (int k = 0; k < Net::NCOND; ++k) s = fmaf(w[k], cvec[k], s);
            v += s;
        } else if ((DIRS || Net::D0_EXPR) && i >= Net::B_D0 && i < Net::B_D0 + 128) {      // near / far fold first, then the expression
            float s = 0.0f;
            if (DIRS) {
                const float* w = packed + Net::OFF_WCD + (i - Net::B_D0) * 16;
                for (int k = 0; k < 16; ++k) s = fmaf(w[k], dvec[k], s);
            }
            if constexpr (Net::D0_EXPR) {
                const float* we = packed + Net::OFF_WCE + (i - Net::B_D0) * Net::NEXPR;
                for (int k = 0; k < Net::NEXPR; ++k) s = fmaf(we[k], cvec[k], s);
            }
            v += s;
        }
        cond[i] = v;
    }
}

template <class Net>
static inline dim3 nf_paper_net_condition_grid() { return dim3((Net::COND_FLOATS + 255) / 256); }

// =================================================================================================
// forward
// =================================================================================================
// the PE part of layers_xyz.3 : [PE | h] -> 256 (skip connection): four register chunks in front of the 16 slab chunks
#define NF_NET_L3_PE()                                                                                        \
    do {                                                                                                      \
        NF_NET_PE_B(0); nf_chunk<NT, 16, true>(acc, st.wa, bj, st.bias);                                          \
        nf_load_w16<16>(st.wa, Wi, Net::OFF_L3 / 4 + 4 * 16 * 64, lane);   /* the first slab chunk, three chunks ahead */ \
        nf_read_b<NT>(st.b0, act4, lane, 0);                                                                  \
        f32x4 w[16];                                                                                          \
        nf_load_w16<16>(w, Wi, Net::OFF_L3 / 4 + 1 * 16 * 64, lane);                                          \
        NF_NET_PE_B(1); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);                                             \
        nf_load_w16<16>(w, Wi, Net::OFF_L3 / 4 + 2 * 16 * 64, lane);                                          \
        NF_NET_PE_B(2); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);                                             \
        nf_load_w16<16>(w, Wi, Net::OFF_L3 / 4 + 3 * 16 * 64, lane);                                          \
        NF_NET_PE_B(3); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);                                             \
    } while (0)

// The colour layers, layers_dir.0 to fc_rgb, as stream text (locals acc / st / bj / dirf / sigma_raw / D0 / NDIR): the end of
// nf_paper_net_body, and what k_paper_mlp_fwd_live (nf_mlp_live.hip) runs on the rows it has gathered.  Entry: feat in the slab;
// layers_dir.0's bias in st.bias, its first weight chunk in st.wa and its first B fragment, as stored, in st.b0 -- what fc_feat's
// nf_tail leaves.  Leaves rgb_raw in acc[t][0].xyz and sigma_raw in sigma_raw[t].
// NF_NET_COLOUR_D0: layers_dir.0 alone, with its first dir-slot chunk's weights already requested into WD_.  NO0_ output tiles are
// computed -- 9: with tile 8, whose row 0 is fc_alpha(feat) and ends up in sigma_raw[t]; 8: without it, sigma_raw is left alone --
// from a weight section whose chunks are WS0_ tiles long (the packed image: 9).  Output tiles are independent MFMA chains: tiles
// 0 .. 7 come out the same either way.
#define NF_NET_COLOUR_D0(NO0_, WS0_, WD_)                                                                                  \
    /* ---- layers_dir.0 : [feat | dir slots] -> 128; tile 8 row 0 = fc_alpha(feat) (Q2) ---- */                            \
    {                                                                                                                      \
        nf_seg_lds<NT, NO0_, true, false, WS0_>(acc, st, Wi, D0, 16, act4, lane);                                          \
        nf_pending_b<NT, false>(bj, st);                                                                                   \
        nf_chunk<NT, NO0_, false>(acc, st.wb, bj, st.bias);                                                                \
        if (NDIR == 2) {                                                                                                   \
            nf_load_w16<NO0_>(st.wb, Wi, D0 + 17 * (WS0_) * 64, lane);                                                     \
            _Pragma("unroll") for (int t = 0; t < NT; ++t) bj[t] = dirf[t][0];                                             \
            nf_chunk<NT, NO0_, false>(acc, WD_, bj, st.bias);                                                              \
        }                                                                                                                  \
        _Pragma("unroll") for (int t = 0; t < NT; ++t) bj[t] = dirf[t][NDIR - 1];                                          \
        if constexpr (NDIR == 2) nf_tail<NT, NO0_, 8, 8, 1>(acc, st.wb, bj, st, Wi, Net::OFF_D1 / 4, Ci, Net::B_D1, act4, lane); \
        else nf_tail<NT, NO0_, 8, 8, 1>(acc, WD_, bj, st, Wi, Net::OFF_D1 / 4, Ci, Net::B_D1, act4, lane);                  \
        if constexpr ((NO0_) > 8) { _Pragma("unroll") for (int t = 0; t < NT; ++t) sigma_raw[t] = acc[t][8].x; }           \
    }
#define NF_NET_COLOUR()                                                                                                    \
    {                                                                                                                      \
        f32x4 wd[16];                                                                                                      \
        nf_load_w16<9>(wd, Wi, D0 + 16 * 9 * 64, lane);                     /* the first dir-slot chunk's weights, a layer ahead */ \
        NF_NET_COLOUR_D0(9, 9, wd);                                                                                        \
    }                                                                                                                      \
    NF_NET_COLOUR_REST()
#define NF_NET_COLOUR_REST()                                                                                               \
    /* ---- layers_dir.1, .2 ---- */                                                                                       \
    nf_seg_lds<NT, 8, true, true>(acc, st, Wi, Net::OFF_D1 / 4, 8, act4, lane);                                            \
    nf_pending_b<NT, true>(bj, st);                                                                                        \
    nf_tail<NT, 8, 8, 8, 1>(acc, st.wb, bj, st, Wi, Net::OFF_D2 / 4, Ci, Net::B_D2, act4, lane);                           \
    nf_seg_lds<NT, 8, true, true>(acc, st, Wi, Net::OFF_D2 / 4, 8, act4, lane);                                            \
    nf_pending_b<NT, true>(bj, st);                                                                                        \
    nf_tail<NT, 8, 8, 1, 1>(acc, st.wb, bj, st, Wi, Net::OFF_RGB / 4, Ci, Net::B_RGB, act4, lane);                         \
    /* ---- fc_rgb ---- */                                                                                                 \
    nf_seg_lds<NT, 1, true, true>(acc, st, Wi, Net::OFF_RGB / 4, 8, act4, lane);                                           \
    nf_pending_b<NT, true>(bj, st);                                                                                        \
    nf_chunk<NT, 1, false>(acc, st.wb, bj, st.bias)

// The network from layers_xyz.0 to fc_rgb on the inference schedule, shared by the ray-input kernels and the pre-encoded ones:
// every layer ends in nf_tail (raw accumulators to the slab tile by tile under the last chunk's MFMAs, the next layer's bias, first
// weights and first B fragment fetched), every layer starts with the bias as the C operand of its first MFMAs, the ReLU is applied
// where the slab is read.  NDIR register chunks of direction slots (1: (sin, cos)(rd_z 2^g), weights OFF_D0; 2: the 24 reference
// columns, weights OFF_D0E) follow layers_dir.0's 16 feat chunks.  Leaves rgb_raw in acc[t][0].xyz and sigma_raw in sigma_raw[t].
// SIGMA: the density-only forward.  Behind fc_feat only fc_alpha runs -- tile 8 of layers_dir.0 over its 16 feat chunks, the same
// MFMAs in the same order as the full layer issues for acc[t][8]; the direction chunk, whose alpha row is zero, and everything
// behind the layer are neither fetched nor issued.  Leaves sigma_raw[t]; acc[t][0] is not a colour.  While that tile runs alone the
// other accumulator tiles are dead: `pre` (SIGMA only) may request what the caller wants next -- pre.wait() stands in front of
// fc_alpha's weight loads, pre.loads() behind them (k_paper_mlp_fwd_live, nf_mlp_live.hip; NfNoPre: nothing).
// GATE (with SIGMA; a family with layers_xyz.5): the trunk ends one layer earlier.  Behind layers_xyz.5 one tile of 16 rows runs
// alone over relu(layers_xyz.5) -- the sigma-bound tile of pre.image() (nf_mlp_gated.hip: rows 0 and 1 are the folded fc_alpha . fc_feat
// and its absolute-value twin, its bias fragment follows its 16 chunks) -- where SIGMA runs fc_alpha's; fc_feat is not issued.  Leaves
// the tile in acc[t][8] (lane group 0: .x = row 0, .y = row 1 of point 16 t + c) and layers_xyz.5's accumulators, as stored, in the slab.
struct NfNoPre {
    __device__ __forceinline__ void wait() const {}
    __device__ __forceinline__ void loads(const NfW&, const NfW&, int) const {}
};
#define NF_BOUND_BIAS 4096                                    // float offset of the bound image's bias fragment (row r of the tile at + r)
#define NF_BOUND_FLOATS (NF_BOUND_BIAS + 16)
// One tile of 16 output rows alone over the slab's 16 chunks (weights: f32x4 index first4 + ch * stride4 of W, chunk 0 already in
// st.wa[0], bias in st.bias[0], first B fragment in st.b0), into acc[t][8].  The other accumulator tiles are dead meanwhile: pre.wait()
// stands in front of the tile's weight loads, pre.loads() behind them.
template <int NT, bool RELU_IN, class Pre>
__device__ __forceinline__ void nf_net_lone_tile(f32x4 (&acc)[NT][16], const NfStream<NT>& st, f32x4 (&bj)[NT], const NfW& W, unsigned first4,
                                                 unsigned stride4, const NfW& Wi, const NfW& Ci, const f32x4* act4, int lane, Pre& pre) {
    f32x4 w8[16];
    w8[0] = st.wa[0];
    pre.wait();
#pragma unroll
    for (int ch = 1; ch < 16; ++ch) w8[ch] = nf_load_w1(W, first4 + stride4 * ch, lane);
    if constexpr (RELU_IN) __builtin_amdgcn_sched_barrier(0);     // (the tile's own weights come back first: loads return in order)
    pre.loads(Wi, Ci, lane);
    if constexpr (RELU_IN) {
        // (GATE only.)  With two MFMA chains in flight nothing hides a chunk's LDS read or its eight v_max if they stand between two
        // chunks, as the plain order below leaves them (profiles/sigma_gate_fine.md: 2,500 clocks per pass against the tile without
        // ReLU).  So chunk ch + 1 is read in front of chunk ch's MFMAs and its ReLU is dealt out among the chunk's last four.  The
        // MFMAs, their operands and their order per accumulator are the plain loop's.
        f32x4 cur[NT], nxt[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) cur[t] = nf_relu_i(st.b0[t]);
#pragma unroll
        for (int ch = 0; ch < 16; ++ch) {
            if (ch + 1 < 16) nf_read_b<NT>(nxt, act4, lane, ch + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[t][8] = __builtin_amdgcn_mfma_f32_16x16x4f32(w8[ch][r], cur[t][r], (ch == 0 && r == 0) ? st.bias[0] : acc[t][8], 0, 0, 0);
#pragma unroll
            for (int r = 2; r < 4; ++r)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (ch + 1 < 16) {
                        const int e = 2 * (r - 2);         // two of the next fragment's four values per MFMA
#pragma unroll
                        for (int q = e; q < e + 2; ++q) {
                            const int xi = __float_as_int(nxt[t][q]);
                            nxt[t][q] = __int_as_float(xi > 0 ? xi : 0);                 // v_max_i32, as nf_relu_i
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    acc[t][8] = __builtin_amdgcn_mfma_f32_16x16x4f32(w8[ch][r], cur[t][r], acc[t][8], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < NT; ++t) cur[t] = nxt[t];
        }
        return;
    }
#pragma unroll
    for (int ch = 0; ch < 16; ++ch) {
        if (ch == 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t) bj[t] = RELU_IN ? nf_relu_i(st.b0[t]) : st.b0[t];
        } else {
            nf_read_b<NT>(bj, act4, lane, ch);
            if (RELU_IN) {
#pragma unroll
                for (int t = 0; t < NT; ++t) bj[t] = nf_relu_i(bj[t]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t][8] = __builtin_amdgcn_mfma_f32_16x16x4f32(w8[ch][r], bj[t][r], (ch == 0 && r == 0) ? st.bias[0] : acc[t][8], 0, 0, 0);
    }
}
template <class Net, int NT, int NDIR, bool SIGMA = false, class Pre = NfNoPre, bool GATE = false>
__device__ __forceinline__ void nf_paper_net_body(f32x4 (&acc)[NT][16], float (&sigma_raw)[NT], const f32x4 (&pe)[NT][4],
                                                  const f32x4 (&dirf)[NT][NDIR], const NfW& Wi, const NfW& Ci, f32x4* act4, int lane,
                                                  Pre pre = Pre()) {
    static_assert(!GATE || (SIGMA && Net::HAS_L5), "the bound tile stands in for fc_alpha's lone tile, behind layers_xyz.5");
    constexpr unsigned D0 = (NDIR == 1 ? Net::OFF_D0 : Net::OFF_D0E) / 4;
    NfStream<NT> st;
    f32x4 bj[NT];
    // one 256-wide layer from the slab (ReLU of the previous layer on read), then the tail that fetches the next layer
#define NF_NET_LAYER256(OFF_, FIRST_, OFF_NEXT_, B_NEXT_, NO_NEXT_, NEXT_B_)                                                \
    nf_seg_lds<NT, 16, FIRST_, true>(acc, st, Wi, OFF_, 16, act4, lane);                                                    \
    nf_pending_b<NT, true>(bj, st);                                                                                         \
    nf_tail<NT, 16, 16, NO_NEXT_, NEXT_B_>(acc, st.wb, bj, st, Wi, OFF_NEXT_, Ci, B_NEXT_, act4, lane)
    NF_NET_PE_LAYER(Net::B_L0, Net::OFF_L0, Net::OFF_L1, Net::B_L1);
    NF_NET_LAYER256(Net::OFF_L1 / 4, true, Net::OFF_L2 / 4, Net::B_L2, 16, 1);
    NF_NET_LAYER256(Net::OFF_L2 / 4, true, Net::OFF_L3 / 4, Net::B_L3, 16, 0);
    NF_NET_L3_PE();
    NF_NET_LAYER256(Net::OFF_L3 / 4 + 4 * 16 * 64, false, Net::OFF_L4 / 4, Net::B_L4, 16, 1);
    if constexpr (GATE) {
        NF_NET_LAYER256(Net::OFF_L4 / 4, true, Net::OFF_L5 / 4, Net::B_L5, 16, 1);
        const NfW Bi = pre.image();
        nf_seg_lds<NT, 16, true, true>(acc, st, Wi, Net::OFF_L5 / 4, 16, act4, lane);
        nf_pending_b<NT, true>(bj, st);
        nf_tail<NT, 16, 16, 1, 1>(acc, st.wb, bj, st, Bi, 0, Bi, NF_BOUND_BIAS, act4, lane);
        nf_net_lone_tile<NT, true>(acc, st, bj, Bi, 0, 64, Wi, Ci, act4, lane, pre);
        return;
    } else if constexpr (Net::HAS_L5) {
        NF_NET_LAYER256(Net::OFF_L4 / 4, true, Net::OFF_L5 / 4, Net::B_L5, 16, 1);
        NF_NET_LAYER256(Net::OFF_L5 / 4, true, Net::OFF_FEAT / 4, Net::B_FEAT, 16, 1);
    } else {
        NF_NET_LAYER256(Net::OFF_L4 / 4, true, Net::OFF_FEAT / 4, Net::B_FEAT, 16, 1);
    }
    // fc_feat (no activation: layers_dir.0 reads it as stored)
    if constexpr (SIGMA) {
        NF_NET_LAYER256(Net::OFF_FEAT / 4, true, D0 + 8 * 64, Net::B_D0 + 128, 1, 1);      // next: tile 8 alone, its bias fragment
        nf_net_lone_tile<NT, false>(acc, st, bj, Wi, D0 + 8 * 64, 9 * 64, Wi, Ci, act4, lane, pre);
#pragma unroll
        for (int t = 0; t < NT; ++t) sigma_raw[t] = acc[t][8].x;
        return;
    }
    NF_NET_LAYER256(Net::OFF_FEAT / 4, true, D0, Net::B_D0, 9, 1);
#undef NF_NET_LAYER256
    NF_NET_COLOUR();
}

// The pre-encoded forward of one wave (model.forward(x87, ...); inference only, the hot path never materialises x): same body,
// inputs from x87, layers_dir.0 with its 24 direction columns as two register chunks, bias table without the direction fold.
template <class Net, int NT>
__device__ __forceinline__ void nf_paper_net_fwd_encoded(f32x4* lds, const float* __restrict__ packed, const float* __restrict__ cond,
                                                         const float* __restrict__ x87, int64_t n_points, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p0 = ((int64_t)blockIdx.x * NF_MLP_WAVES + wave) * (16 * NT);
    if (p0 >= n_points) return;
    f32x4* act4 = lds + wave * (16 * NT * 64);
    f32x4 pe[NT][4];
    f32x4 dirf[NT][2];
    nf_net_inputs_encoded<NT>(pe, dirf, p0, n_points, lane, x87);
    f32x4 acc[NT][16];
    float sigma_raw[NT];
    const NfW Wi = nf_w_image(packed, Net::PACKED), Ci = nf_w_image(cond, Net::COND_FLOATS);
    nf_paper_net_body<Net, NT, 2>(acc, sigma_raw, pe, dirf, Wi, Ci, act4, lane);
    nf_net_store_raw<NT>(acc, sigma_raw, p0, n_points, lane, out);
}

// x87: (n_points, 87) pre-encoded inputs; cond: scratch of the family's cond_floats; out: (n_points, 4).  `condition` / `forward`: the
// family's k_*_condition (without the direction fold) and k_*_mlp_fwd_encoded<NF_MLP_NT> launchers.
template <class Condition, class Forward>
static inline int nf_paper_net_forward_encoded(const float* packed, const float* x87, const float* expr76, const float* latent32,
                                               int64_t n_points, float* cond, float* out, Condition condition, Forward forward) {
    if (n_points == 0) return 0;                           // nothing to do (empty tensors have NULL data pointers)
    if (!packed || !x87 || !expr76 || !latent32 || !cond || !out || n_points < 0) return NF_EINVAL;
    condition();
    const int64_t per_block = (int64_t)NF_MLP_WAVES * 16 * NF_MLP_NT;
    const int64_t grid = (n_points + per_block - 1) / per_block;
    if (grid > 0x7fffffff) return NF_EINVAL;
    forward((unsigned)grid);
    NF_RETURN_LAUNCH();
}

// Training forward of one wave (exact f32): the same arithmetic as nf_paper_net_body, plus everything the backward needs in `saved`
// (layout Net::S_*): every layer output as row-major [n][width] matrices for the weight-gradient GEMMs -- copied out of the wave's
// LDS slab as whole 128-byte lines from inside the NEXT layer's K loop -- and the ReLU bit masks the dX chain applies (8 bytes per
// lane, tile and layer).  Everything is produced where the slab is READ, inside the K loops: the loop that consumes a layer's output
// applies the ReLU to its B fragments, collects their [x > 0] bits (nf_mask_bits -- a lane reads back exactly the elements it wrote)
// and carries the copy of the slab to `saved`, ReLU applied on the way out (NfCopyH: four whole-line stores per step of two chunks).
template <class Net, int NT>
__device__ __forceinline__ void nf_paper_net_body_save(f32x4 (&acc)[NT][16], float (&sigma_raw)[NT], const f32x4 (&pe)[NT][4],
                                                       const f32x4 (&dirf)[NT][1], const NfW& Wi, const NfW& Ci, f32x4* act4, int lane,
                                                       float* __restrict__ saved, int64_t p0, int64_t n) {
    static_assert(NT == 2, "the copy schedule below is written for 32-point slabs");
    constexpr int NX = nf_net_n_xyz<Net>;
    const int g = lane >> 4, c = lane & 15;
    auto sec = [&](int s, int width) { return nf_slab_copy(saved, s, width, p0, n); };
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int64_t p = p0 + 16 * t + c;
        // dir slots: 64 B per point, the 16 points of a tile are one contiguous KiB
        if (p < n) *reinterpret_cast<f32x4*>(saved + Net::S_DIRF * n + p * 16 + 4 * g) = dirf[t][0];
#pragma unroll
        for (int j = 0; j < 4; ++j) act4[nf_act_idx4(16 * t + c, 4 * j + g)] = pe[t][j];       // PE slots 16 j + 4 g .. + 3
    }
    {   // PE rows (64 slots = 256 B per point): four rows per instruction, before layers_xyz.0's output takes the slab
        const NfSlabCopy cp = sec(Net::S_PE, 64);
#pragma unroll
        for (int k = 0; k < 16 * NT / 4; ++k) nf_copy_rows<16>(act4, cp, k, lane);
    }
    uint64_t m64[NT];
    NfStream<NT> st;
    f32x4 bj[NT];
    // one 128-wide layer's K loop (two rows per copy instruction); its tail follows
#define NF_NET_LAYER128(OFF_, NO_, SEC_, MASKL_)                                                                          \
    NfCopyH<32, 4, true> cs{act4, sec(SEC_, 128), lane, 4, {}};                                                            \
    cs.prime();                                                                                                            \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) m64[t] = 0;                                                             \
    nf_seg_lds<NT, NO_, true, true, true>(acc, st, Wi, OFF_, 8, act4, lane, cs, m64);                                      \
    NF_NET_SAVE_PENDING(true, MASKL_, 8)
    NF_NET_PE_LAYER(Net::B_L0, Net::OFF_L0, Net::OFF_L1, Net::B_L1);
    // ---- layers_xyz.1, .2 (each K loop also streams the layer output it consumes to `saved`), .3 (skip), .4 (, .5), fc_feat ------
    NF_NET_SAVE_LAYER256(Net::OFF_L1 / 4, true, Net::S_H0, 0, Net::OFF_L2 / 4, Net::B_L2, 16, 1);
    NF_NET_SAVE_LAYER256(Net::OFF_L2 / 4, true, Net::S_H1, 1, Net::OFF_L3 / 4, Net::B_L3, 16, 0);
    NF_NET_L3_PE();
    NF_NET_SAVE_LAYER256(Net::OFF_L3 / 4 + 4 * 16 * 64, false, Net::S_H2, 2, Net::OFF_L4 / 4, Net::B_L4, 16, 1);
    if constexpr (Net::HAS_L5) {
        NF_NET_SAVE_LAYER256(Net::OFF_L4 / 4, true, Net::S_H3, 3, Net::OFF_L5 / 4, Net::B_L5, 16, 1);
        NF_NET_SAVE_LAYER256(Net::OFF_L5 / 4, true, Net::S_H4, 4, Net::OFF_FEAT / 4, Net::B_FEAT, 16, 1);
        NF_NET_SAVE_LAYER256(Net::OFF_FEAT / 4, true, Net::S_H5, 5, Net::OFF_D0 / 4, Net::B_D0, 9, 1);
    } else {
        NF_NET_SAVE_LAYER256(Net::OFF_L4 / 4, true, Net::S_H3, 3, Net::OFF_FEAT / 4, Net::B_FEAT, 16, 1);
        NF_NET_SAVE_LAYER256(Net::OFF_FEAT / 4, true, Net::S_H4, 4, Net::OFF_D0 / 4, Net::B_D0, 9, 1);
    }
    // ---- layers_dir.0 : [feat | dir slots] -> 128; tile 8 row 0 = fc_alpha(feat) (Q2); fc_feat has no activation ------------------
    {
        f32x4 wd[16];
        nf_load_w16<9>(wd, Wi, Net::OFF_D0 / 4 + 16 * 9 * 64, lane);        // the dir-slot chunk's weights, a layer ahead
        NfCopyH<64, 4, false> cs{act4, sec(Net::S_FEAT, 256), lane, 8, {}};
        cs.prime();
        nf_seg_lds<NT, 9, true, false, false>(acc, st, Wi, Net::OFF_D0 / 4, 16, act4, lane, cs, m64);
        NF_NET_SAVE_PENDING(false, -1, 16);
        nf_chunk<NT, 9, false>(acc, st.wb, bj, st.bias);
#pragma unroll
        for (int t = 0; t < NT; ++t) bj[t] = dirf[t][0];
        nf_tail<NT, 9, 8, 8, 1>(acc, wd, bj, st, Wi, Net::OFF_D1 / 4, Ci, Net::B_D1, act4, lane);
#pragma unroll
        for (int t = 0; t < NT; ++t) sigma_raw[t] = acc[t][8].x;
    }
    // ---- layers_dir.1, .2, fc_rgb ----------------------------------------------------------------------------------------------
    {
        NF_NET_LAYER128(Net::OFF_D1 / 4, 8, Net::S_D0, NX);
        nf_tail<NT, 8, 8, 8, 1>(acc, st.wb, bj, st, Wi, Net::OFF_D2 / 4, Ci, Net::B_D2, act4, lane);
    }
    {
        NF_NET_LAYER128(Net::OFF_D2 / 4, 8, Net::S_D1, NX + 1);
        nf_tail<NT, 8, 8, 1, 1>(acc, st.wb, bj, st, Wi, Net::OFF_RGB / 4, Ci, Net::B_RGB, act4, lane);
    }
    {
        NF_NET_LAYER128(Net::OFF_RGB / 4, 1, Net::S_D2, NX + 2);
        nf_chunk<NT, 1, false>(acc, st.wb, bj, st.bias);
    }
#undef NF_NET_LAYER128
}
#undef NF_NET_L3_PE

template <class Net, int NT>
__device__ __forceinline__ void nf_paper_net_fwd_save(f32x4* lds, const float* __restrict__ packed, const float* __restrict__ cond,
                                                      const float* __restrict__ ro, const float* __restrict__ rd,
                                                      const float* __restrict__ rd_view, const float* __restrict__ z, int64_t n_points, int S,
                                                      float* __restrict__ raw, float* __restrict__ saved) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p0 = ((int64_t)blockIdx.x * NF_MLP_WAVES + wave) * (16 * NT);
    if (p0 >= n_points) return;                       // wave-uniform; no barriers anywhere below
    f32x4* act4 = lds + wave * (16 * NT * 64);
    f32x4 pe[NT][4];
    f32x4 dirf[NT][1];
    nf_net_inputs<NT>(pe, dirf, p0, n_points, S, lane, ro, rd, rd_view, z);
    f32x4 acc[NT][16];
    float sigma_raw[NT];
    const NfW Wi = nf_w_image(packed, Net::PACKED), Ci = nf_w_image(cond, Net::COND_FLOATS);
    nf_paper_net_body_save<Net, NT>(acc, sigma_raw, pe, dirf, Wi, Ci, act4, lane, saved, p0, n_points);
    nf_net_store_raw<NT>(acc, sigma_raw, p0, n_points, lane, raw);
}

// Launch of a family's ray-input forward: `fwd` = its k_*_mlp_fwd<NF_MLP_NT> (inference: a persistent grid, at most one workgroup per
// CU), `fwd_save` = its k_*_mlp_fwd_save<NF_MLP_NT> (saved != NULL)
template <class Fwd, class FwdSave>
static inline int nf_paper_net_launch_fwd(Fwd fwd, FwdSave fwd_save, const float* packed, const float* cond, const float* ro, const float* rd,
                                          const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw, float* saved,
                                          nf_stream_t stream) {
    static_assert(NF_MLP_WAVES * 16 * NF_MLP_NT == 128, "nf_mlp_fwd_launch sizes the grid for 128 points per workgroup");
    const float* rdv = rd_view ? rd_view : rd;
    return nf_mlp_fwd_launch(saved ? NF_FWD_TRAIN_F32 : NF_FWD_INFER, packed, cond, ro, rd, z, raw, saved, n_rays, n_samples,
                             [&](int64_t n_points, unsigned grid) {
        if (saved)
            hipLaunchKernelGGL(fwd_save, dim3(grid), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream), packed, cond, ro, rd, rdv, z, n_points,
                               n_samples, raw, saved);
        else
            hipLaunchKernelGGL(fwd, dim3((unsigned)(grid < nf_cu_count() ? grid : nf_cu_count())), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream),
                               packed, cond, ro, rd, rdv, z, n_points, n_samples, raw);
    });
}

// Density-only inference forward of one workgroup (nf_paper_net_body<..., SIGMA>): the persistent block loop of the family's
// k_*_mlp_fwd, one float per point written.  The direction never reaches fc_alpha, so no rd_view is read.
template <class Net, int NT>
__device__ __forceinline__ void nf_paper_net_fwd_sigma(f32x4* lds, const float* __restrict__ packed, const float* __restrict__ cond_,
                                                       const float* __restrict__ ro, const float* __restrict__ rd, const float* __restrict__ z,
                                                       int64_t n_points, int S, float* __restrict__ sigma) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15;
    f32x4* act4 = lds + wave * (16 * NT * 64);
    typedef __attribute__((address_space(1))) float nf_gf32;
    nf_gf32* sigma_v = (nf_gf32*)sigma;               // the output pointer and the grid stride live in VGPRs, as in k_paper_mlp_fwd
    asm volatile("" : "+v"(sigma_v));
    int stride_v = (int)gridDim.x;
    asm volatile("" : "+v"(stride_v));
    const float* z_v = z;                             // (and the depths' pointer: the last scalar pair the block loop could not keep)
    asm volatile("" : "+v"(z_v));
#pragma unroll 1
    for (int64_t blk = blockIdx.x;; blk += __builtin_amdgcn_readfirstlane(stride_v)) {
        const int64_t p0 = (blk * NF_MLP_WAVES + wave) * (16 * NT);
        if (p0 >= n_points) break;                    // wave-uniform; no barriers anywhere below
        int opaque0 = 0;                              // per-block opaque zero: the weight / bias loads must stay where the layers issue them
        asm volatile("" : "+s"(opaque0));
        const float* W = packed + opaque0;
        const float* cond = cond_ + opaque0;
        f32x4 pe[NT][4];
        f32x4 dirf[NT][1];
        nf_net_inputs<NT>(pe, dirf, p0, n_points, S, lane, ro, rd, rd, z_v);
        f32x4 acc[NT][16];
        float sigma_raw[NT];
        const NfW Wi = nf_w_image(W, Net::PACKED), Ci = nf_w_image(cond, Net::COND_FLOATS);
        nf_paper_net_body<Net, NT, 1, true>(acc, sigma_raw, pe, dirf, Wi, Ci, act4, lane);
        int lane_o = lane;
        asm volatile("" : "+v"(lane_o));
        if ((lane_o >> 4) == 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int64_t p = p0 + 16 * t + c;
                if (p < n_points) sigma_v[p] = sigma_raw[t];
            }
        }
    }
}

// Launch of a family's k_*_mlp_sigma<NF_MLP_NT> (a persistent grid, at most one workgroup per CU); checks as the full forward's
template <class Sigma>
static inline int nf_paper_net_launch_sigma(Sigma kernel, const float* packed, const float* cond, const float* ro, const float* rd,
                                            const float* z, int64_t n_rays, int n_samples, float* sigma, nf_stream_t stream) {
    static_assert(NF_MLP_WAVES * 16 * NF_MLP_NT == 128, "nf_mlp_fwd_launch sizes the grid for 128 points per workgroup");
    return nf_mlp_fwd_launch(NF_FWD_INFER, packed, cond, ro, rd, z, sigma, nullptr, n_rays, n_samples, [&](int64_t n_points, unsigned grid) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)(grid < nf_cu_count() ? grid : nf_cu_count())), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream),
                           packed, cond, ro, rd, z, n_points, n_samples, sigma);
    });
}
