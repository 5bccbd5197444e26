// The two blendshape classes without a learnable code (reference nerf/models.py: ConditionalBlendshapeNeRFModel M:872-976,
// ConditionalCompressedBlendshapeNeRFModel M:750-868) run on the second family's per-point kernels: per point they ARE that
// network.  What differs is constant per call -- the vector folded into layer1's bias -- so each class owns its gather tables
// (built by the second family's builders for its geometry), its condition kernel and its gradient scatter -- both wrappers of the
// family's trunk (nf_mlp_lcode_net.h, nf_mlp_lcode_net_bwd.h); everything per point is launched through the nf_lcode_* entry points
// on images laid out as nf_mlp_lcode_layout.h says.
#pragma once
#include "nf_mlp_lcode_net_bwd.h"

// ---- the compressed class: tail of its packed f32 image (the expression encoder, row-major) and its corner of `cond` ----
namespace ncb {
constexpr int N_ENC = 6;                                   // layers_expr.0..2 (weight, bias) in front of the 16 trunk tensors
constexpr int NPARAMS = N_ENC + nlc::NPARAMS;
constexpr int D0 = 76, D1 = 38, D2 = 20, D3 = 20;          // expr -> e1 -> e2 -> e3, a ReLU after each layer (M:832-834)
constexpr int E_W0 = 0, E_B0 = E_W0 + D1 * D0, E_W1 = E_B0 + D1, E_B1 = E_W1 + D2 * D1, E_W2 = E_B1 + D2, E_B2 = E_W2 + D3 * D2;
constexpr int ENC_FLOATS = E_B2 + D3;                      // 4126 = the six tensors, also the head of the gradient vector
constexpr int OFF_ENC = nlc::PACKED;
constexpr int PACKED = OFF_ENC + ((ENC_FLOATS + 3) & ~3);
// behind B_DVEC + 16 of the 2560-float bias table: the encoder's input and its three outputs, for the backward
constexpr int C_EXPR = nlc::COND_FLOATS, C_E1 = C_EXPR + D0, C_E2 = C_E1 + D1, C_E3 = C_E2 + D2, C_END = C_E3 + D3;
static_assert(C_END <= 2560, "the encoder's activations must fit the padded bias table");
constexpr int LD1 = 63 + D3;
constexpr int GRAD_PARAM_FLOATS = ENC_FLOATS + nlc::GRAD_PARAM_FLOATS - 256 * (171 - LD1);
}  // namespace ncb

namespace nbs {
constexpr int N_EXPR = 76;
constexpr int LD1 = 63 + N_EXPR;
constexpr int GRAD_PARAM_FLOATS = nlc::GRAD_PARAM_FLOATS - 256 * (171 - LD1);
}  // namespace nbs

// Every entry point of a class that is the second family's on the class's own images, and the six pack entry points.
// PFX: nf_bshape / nf_cbshape; GEOM: the class's NfLcodeGeom; NP: its parameter count; TAG: keeps the pack kernels' instantiations
// apart; TABLE_F32: builder of the class's exact-f32 table (the trunk table, plus the class's tail); PACKED_F32: its size.
#define NF_BSHAPE_SHARED_ENTRY_POINTS(PFX, GEOM, NP, TAG, TABLE_F32, PACKED_F32)                                                          \
    static NfPackTable PFX##_tab_f32, PFX##_tab_t, PFX##_tab_b, PFX##_tab_bt, PFX##_tab_h, PFX##_tab_ht;                                  \
    static void PFX##_table_t(std::vector<uint32_t>& t) { nf_lcode_build_table_t(t, GEOM); }                                             \
    static void PFX##_table_bf16(std::vector<uint32_t>& t) { nf_lcode_build_table_bf16(t, GEOM); }                                       \
    static void PFX##_table_bf16_t(std::vector<uint32_t>& t) { nf_lcode_build_table_bf16_t(t, GEOM); }                                   \
    extern "C" size_t PFX##_packed_floats(void) { return (size_t)(PACKED_F32); }                                                          \
    extern "C" size_t PFX##_cond_floats(void) { return nf_lcode_cond_floats(); }                                                          \
    extern "C" int PFX##_pack(const float* const* params, float* packed, nf_stream_t stream) {                                            \
        return nf_pack_f32<NP, TAG>(PFX##_tab_f32, TABLE_F32, params, packed, (int)(PACKED_F32), stream);                                 \
    }                                                                                                                                     \
    extern "C" size_t PFX##_packed_bwd_floats(void) { return nf_lcode_packed_bwd_floats(); }                                              \
    extern "C" int PFX##_pack_bwd(const float* const* params, float* packed_t, nf_stream_t stream) {                                      \
        return nf_pack_f32<NP, TAG + 1>(PFX##_tab_t, PFX##_table_t, params, packed_t, (int)nlc::PACKED_T, stream);                        \
    }                                                                                                                                     \
    extern "C" size_t PFX##_packed_bf16_bytes(void) { return nf_lcode_packed_bf16_bytes(); }                                              \
    extern "C" int PFX##_pack_bf16(const float* const* params, void* out, nf_stream_t stream) {                                           \
        return nf_pack_split_bf16<NP, TAG + 2>(PFX##_tab_b, PFX##_table_bf16, params, out, (int)(nf_lcode_packed_bf16_bytes() / 4), stream); \
    }                                                                                                                                     \
    extern "C" size_t PFX##_packed_bwd_bf16_bytes(void) { return nf_lcode_packed_bwd_bf16_bytes(); }                                      \
    extern "C" int PFX##_pack_bwd_bf16(const float* const* params, void* out, nf_stream_t stream) {                                       \
        return nf_pack_split_bf16<NP, TAG + 3>(PFX##_tab_bt, PFX##_table_bf16_t, params, out, (int)(nf_lcode_packed_bwd_bf16_bytes() / 4), \
                                               stream);                                                                                   \
    }                                                                                                                                     \
    extern "C" size_t PFX##_packed_f16_bytes(void) { return nf_lcode_packed_f16_bytes(); }                                                \
    extern "C" size_t PFX##_f16_flag_offset(void) { return nf_lcode_f16_flag_offset(); }                                                  \
    extern "C" int PFX##_pack_f16(const float* const* params, void* out, nf_stream_t stream) {                                            \
        NfLayerPairs<8> lp;                                                                                                               \
        const float act_scale = nf_lcode_f16_stream_layers(lp.off);                                                                       \
        return nf_pack_split_f16<NP, TAG + 4, 8>(PFX##_tab_h, PFX##_table_bf16, params, out, lp.off[8] * 512, lp, act_scale, stream);     \
    }                                                                                                                                     \
    extern "C" size_t PFX##_packed_bwd_f16_bytes(void) { return nf_lcode_packed_bwd_f16_bytes(); }                                        \
    extern "C" int PFX##_pack_bwd_f16(const float* const* params, void* out, nf_stream_t stream) {                                        \
        NfLayerPairs<6> lp;                                                                                                               \
        nf_lcode_bwd_f16_stream_layers(lp.off);                                                                                           \
        return nf_pack_split_f16<NP, TAG + 5, 6>(PFX##_tab_ht, PFX##_table_bf16_t, params, out, lp.off[6] * 512, lp, 1.0f, stream);       \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,          \
                                 const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream) {                         \
        return nf_lcode_mlp_fwd(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, stream);                                        \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_fwd_bf16(const void* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,      \
                                      const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream) {                    \
        return nf_lcode_mlp_fwd_bf16(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, stream);                                   \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_fwd_f16(const void* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,       \
                                     const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream) {                     \
        return nf_lcode_mlp_fwd_f16(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, stream);                                    \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_fwd_f16x2(const void* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,     \
                                       const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream) {                   \
        return nf_lcode_mlp_fwd_f16x2(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, stream);                                  \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_sigma(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,        \
                                   const float* z, int64_t n_rays, int n_samples, float* sigma, nf_stream_t stream) {                     \
        return nf_lcode_mlp_sigma(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, sigma, stream);                                    \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_sigma_bf16(const void* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,    \
                                        const float* z, int64_t n_rays, int n_samples, float* sigma, nf_stream_t stream) {                \
        return nf_lcode_mlp_sigma_bf16(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, sigma, stream);                               \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_sigma_f16(const void* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,     \
                                       const float* z, int64_t n_rays, int n_samples, float* sigma, nf_stream_t stream) {                 \
        return nf_lcode_mlp_sigma_f16(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, sigma, stream);                                \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_sigma_f16x2(const void* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,   \
                                         const float* z, int64_t n_rays, int n_samples, float* sigma, nf_stream_t stream) {               \
        return nf_lcode_mlp_sigma_f16x2(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, sigma, stream);                              \
    }                                                                                                                                     \
    extern "C" size_t PFX##_saved_floats(int64_t n_points) { return nf_lcode_saved_floats(n_points); }                                    \
    extern "C" int PFX##_mlp_fwd_train(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,    \
                                       const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream) {     \
        return nf_lcode_mlp_fwd_train(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, saved, stream);                           \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_fwd_train_bf16(const void* packed, const float* cond, const float* ro, const float* rd,                      \
                                            const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,              \
                                            float* saved, nf_stream_t stream) {                                                           \
        return nf_lcode_mlp_fwd_train_bf16(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, saved, stream);                      \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_fwd_train_f16(const void* packed, const float* cond, const float* ro, const float* rd,                       \
                                           const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,               \
                                           float* saved, nf_stream_t stream) {                                                            \
        return nf_lcode_mlp_fwd_train_f16(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, saved, stream);                       \
    }                                                                                                                                     \
    extern "C" size_t PFX##_bwd_workspace_floats(int64_t n_points) { return nf_lcode_bwd_workspace_floats(n_points); }                    \
    static int PFX##_bwd(int precision, const float* packed, const void* packed_t, const float* cond, const float* saved,                 \
                         const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads,      \
                         nf_stream_t stream, float* stage_ms = nullptr) {                                                                 \
        static const NfBwdFamily fam = nf_lcode_bwd_family(PFX##_reduce_unpack);                                                          \
        return nf_bwd_run(fam, precision, packed, packed_t, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads,    \
                          stream, stage_ms);                                                                                              \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_bwd_stage_ms(const float* packed, const void* packed_t_any, int precision, const float* cond,                \
                                          const float* saved, const float* d_raw, int64_t n_rays, int n_samples, float* workspace,        \
                                          size_t workspace_floats, float* grads, float* stage_ms, nf_stream_t stream) {                   \
        if (precision < 0 || precision > 2 || !stage_ms) return NF_EINVAL;                                                                \
        return PFX##_bwd(precision, packed, packed_t_any, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads,      \
                         stream, stage_ms);                                                                                               \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_bwd(const float* packed, const float* packed_t, const float* cond, const float* saved, const float* d_raw,   \
                                 int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads,                  \
                                 nf_stream_t stream) {                                                                                    \
        return PFX##_bwd(0, packed, packed_t, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads, stream);         \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_bwd_bf16(const float* packed, const void* packed_t, const float* cond, const float* saved,                   \
                                      const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,       \
                                      float* grads, nf_stream_t stream) {                                                                 \
        return PFX##_bwd(1, packed, packed_t, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads, stream);         \
    }                                                                                                                                     \
    extern "C" int PFX##_mlp_bwd_f16(const float* packed, const void* packed_t, const float* cond, const float* saved,                    \
                                     const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,        \
                                     float* grads, nf_stream_t stream) {                                                                  \
        return PFX##_bwd(2, packed, packed_t, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads, stream);         \
    }
