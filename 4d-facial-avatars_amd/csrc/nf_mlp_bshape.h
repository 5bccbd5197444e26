// The two blendshape classes without a learnable code (reference nerf/models.py: ConditionalBlendshapeNeRFModel M:872-976,
// ConditionalCompressedBlendshapeNeRFModel M:750-868) run on the second family's per-point kernels: per point they ARE that
// network.  What differs is constant per call -- the vector folded into layer1's bias -- so each class owns its gather tables
// (built by the second family's builders for its geometry), its condition kernel and its gradient scatter; everything per
// point is launched through the nf_lcode_* entry points on images laid out as nf_mlp_lcode_layout.h says.
#pragma once
#include <vector>
#include "nf_mlp_lcode_layout.h"
#include "nf_mlp_bwd.h"
#include "nf_pack.h"
#include "../../include/nerface_hip.h"

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

// ---- what the second family's translation units provide -----------------------------------------------------------------
void nf_lcode_build_table(std::vector<uint32_t>& t, const NfLcodeGeom& ge);           // exact-f32 image (nf_mlp_lcode.hip)
void nf_lcode_build_table_t(std::vector<uint32_t>& t, const NfLcodeGeom& ge);         // transposed image (nf_mlp_lcode_bwd.hip)
void nf_lcode_build_table_bf16(std::vector<uint32_t>& t, const NfLcodeGeom& ge);      // (hi, lo) stream (nf_mlp_lcode_bf16.hip)
void nf_lcode_build_table_bf16_t(std::vector<uint32_t>& t, const NfLcodeGeom& ge);    // transposed stream (nf_mlp_lcode_bf16_bwd.hip)
float nf_lcode_f16_stream_layers(int* pair_off);                                      // 8 + 1 offsets; returns the activation pre-scale
void nf_lcode_bwd_f16_stream_layers(int* pair_off);                                   // 6 + 1 offsets
int nf_lcode_launch_fwd_encoded(const float* packed, const float* cond, const float* x87, int64_t n_points, float* out, nf_stream_t stream);
void nf_lcode_grad_reduce(const float* slabs, int ns, const NfReduceAlt& alt, float* sum, hipStream_t s);
NfBwdFamily nf_lcode_bwd_family(void (*reduce_unpack)(const float*, int, const NfReduceAlt&, float*, const float*, const float*, float*,
                                                      hipStream_t));

// One trunk element of the flat gradient vector (the 16 tensors of nerf.ops.LCODE_KEYS order, layer1.weight LD1 columns wide) from the
// reduced slab: k_lcode_grad_unpack's scatter with the class's column count; cvec = the folded vector (cond + B_CVEC).
template <int LD1>
struct NfBsGradOffsets { int off[nlc::NPARAMS + 1]; };

template <int LD1>
static inline NfBsGradOffsets<LD1> nf_bs_grad_offsets() {
    const int numel[nlc::NPARAMS] = {256 * LD1, 256, 65536, 256, 65536, 256, 65536, 256, 128 * 280, 128, 256, 1, 384, 3, 65536, 256};
    NfBsGradOffsets<LD1> o;
    o.off[0] = 0;
    for (int i = 0; i < nlc::NPARAMS; ++i) o.off[i + 1] = o.off[i] + numel[i];
    return o;
}

template <int LD1>
__device__ __forceinline__ float nf_bs_trunk_grad(int e, const NfBsGradOffsets<LD1>& offs, const float* __restrict__ sum,
                                                  const float* __restrict__ cvec, const float* __restrict__ dvec) {
    using namespace nlc;
    int t = 0;
    while (e >= offs.off[t + 1]) ++t;
    const int local = e - offs.off[t];
    switch (t) {
        case 0: {  // layer1.weight [256][LD1] = [pe 63 | folded vector]
            const int n = local / LD1, col = local - LD1 * n;
            return col < 63 ? sum[G_L1 + n * 64 + nfl::pe_col_to_slot(col)] : sum[CS_L1 + n] * cvec[col - 63];
        }
        case 1: return sum[CS_L1 + local];
        case 2: return sum[G_X0 + local];
        case 3: return sum[CS_L1 + 256 + local];
        case 4: return sum[G_X1 + local];
        case 5: return sum[CS_L1 + 512 + local];
        case 6: return sum[G_X2 + local];
        case 7: return sum[CS_L1 + 768 + local];
        case 8: {  // layers_dir.0.weight [128][280] = [feat 256 | PE4(rd_z, near, far) 24]
            const int n = local / 280, col = local - 280 * n;
            if (col < 256) return sum[G_DIRA + n * 256 + col];
            const int q = col - 256, f = q / 6, rem = q - 6 * f, sc = rem / 3, comp = rem - 3 * sc;
            return comp == 0 ? sum[G_DIRB + n * 16 + 4 * f + sc] : sum[CS_DIR + n] * dvec[4 * f + 2 * sc + (comp - 1)];
        }
        case 9: return sum[CS_DIR + local];
        case 10: return sum[G_ALPHA + 3 * 256 + local];      // fc_alpha.weight [1][256] = row 3 (d sigma) of d_raw^T x
        case 11: return sum[CS_RGB + 3];
        case 12: return sum[G_RGB + local];                  // fc_rgb.weight [3][128]
        case 13: return sum[CS_RGB + local];
        case 14: return sum[G_FEAT + local];
        default: return sum[CS_L1 + 1024 + local];
    }
}

// the (near, far) direction features both classes fold into layers_dir.0's bias, as k_lcode_condition forms them
__device__ __forceinline__ float nf_bs_dvec(int k, float near_z, float far_z) {
    const int f = k >> 2, sc = (k >> 1) & 1, comp = k & 1;
    const float a = nf_mul(comp ? far_z : near_z, exp2f((float)f));
    return sc ? cosf(a) : sinf(a);
}

// The bias table from the folded vector cvec[108] (LDS; entries past N_COND are zero) and dvec[16]: k_lcode_condition's loop with the
// class's column count, same fmaf order.  ENCODED: the table of <prefix>_forward_encoded (no direction fold, dvec = 0).
template <int N_COND, bool ENCODED>
__device__ __forceinline__ void nf_bs_bias_table(const float* __restrict__ packed, const float* cvec, const float* dvec,
                                                 float* __restrict__ cond) {
    using namespace nlc;
    const float* bias = packed + OFF_BIAS;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < COND_FLOATS; i += gridDim.x * blockDim.x) {
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
