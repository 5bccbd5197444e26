// Third model family: ConditionalBlendshapePaperSmallerNeRFModel (reference nerf/models.py:266-338) as its two configs
// instantiate it (10 / 4 encoding functions, include_input_dir False, use_viewdirs True) together with run_network's input
// assembly (reference nerf/train_utils.py:9-33,78):
//   x0 = [PE10(xyz) 63 | expr*1/3 76 | latent 32];  3 x relu(Linear 256);  relu(layers_xyz.3([x0 | h]));  relu(layers_xyz.4)
//   feat = fc_feat(h) (no activation);  sigma = fc_alpha(feat);
//   relu(layers_dir.0([feat | PE4(dir) 24 | expr*1/3 76])) -> 2 x relu(Linear 128) -> rgb = fc_rgb
// i.e. the paper model (nf_mlp.hip) without layers_xyz.5 and the dead layers_dir.3, with the expression a second time in front of
// the colour branch.  Exact f32 only.  Same structure as k_paper_mlp_fwd / k_paper_mlp_fwd_save: layer-streamed waves that own 32
// points each (nf_mlp_stream.h), four wave-private 32 KiB LDS slabs, no barrier, weights and biases as buffer loads from the
// fragment-ordered image, the bias as the C operand, the positional encoding resident in registers.  Every per-call constant input
// column -- expression and latent code in layers_xyz.0 / .3, and in layers_dir.0 the expression and PE4(near), PE4(far) -- is
// folded into the bias table by nf_smaller_condition: 6788 MFMAs per 16 points against the paper kernel's 7812.
#include <vector>
#include <mutex>
#include "nf_mlp_dev.h"
#include "nf_mlp_stream.h"
#include "nf_mlp_smaller_layout.h"
#include "nf_pack.h"

// =================================================================================================
// pack: gather the 22 nn.Parameter storages into the fragment-ordered image
// =================================================================================================
// state_dict ids
enum { SM_XYZ0_W = 0, SM_XYZ3_W = 6, SM_FEAT_W = 10, SM_FEAT_B = 11, SM_ALPHA_W = 12, SM_ALPHA_B = 13, SM_DIR0_W = 14, SM_DIR0_B = 15,
       SM_RGB_W = 20, SM_RGB_B = 21 };

static void nf_smaller_table(std::vector<uint32_t>& t) {
    using namespace nsm;
    t.assign(PACKED, NF_ZERO_CODE);
    // col_of(slot) -> reference column of `tensor` (or -1 = zero); rows >= n_out are zero, except that `alpha_row` (if >= 0) is
    // served from fc_alpha.weight (fc_alpha reads feat only: slots 0..255)
    auto fill = [&](int off, int nk, int no_tiles, int tensor, int n_out, int n_cols, auto col_of, int alpha_row = -1) {
        nf_fill_frag(t, off, nk, no_tiles, [&](int slot, int n) {
            if (n < n_out) {
                const int col = col_of(slot);
                return col >= 0 ? nf_code(tensor, n, col, n_cols) : NF_ZERO_CODE;
            }
            return n == alpha_row && slot < 256 ? nf_code(SM_ALPHA_W, 0, slot, 256) : NF_ZERO_CODE;
        });
    };
    auto ident = [](int s) { return s; };
    fill(OFF_L0, 4, 16, SM_XYZ0_W, 256, 171, [](int s) { return nfl::pe_slot_to_col(s); });
    fill(OFF_L1, 16, 16, 2, 256, 256, ident);
    fill(OFF_L2, 16, 16, 4, 256, 256, ident);
    fill(OFF_L3, 20, 16, SM_XYZ3_W, 256, 427, [](int s) { return s < 64 ? nfl::pe_slot_to_col(s) : 171 + (s - 64); });
    fill(OFF_L4, 16, 16, 8, 256, 256, ident);
    fill(OFF_FEAT, 16, 16, SM_FEAT_W, 256, 256, ident);
    // layers_dir.0: slots 0..255 = feat; chunk 16: lane group g holds (sin, cos)(rd_z * 2^g) at r = 0, 1
    fill(OFF_D0, 17, 9, SM_DIR0_W, 128, 356,
         [](int s) {
             if (s < 256) return s;
             const int g = ((s - 256) >> 2) & 3, r = (s - 256) & 3;
             return r < 2 ? 256 + 6 * g + 3 * r : -1;
         },
         /*alpha_row=*/128);
    fill(OFF_D0E, 18, 9, SM_DIR0_W, 128, 356, [](int s) { return s < 280 ? s : -1; }, /*alpha_row=*/128);
    fill(OFF_D1, 8, 8, 16, 128, 128, ident);
    fill(OFF_D2, 8, 8, 18, 128, 128, ident);
    fill(OFF_RGB, 8, 1, SM_RGB_W, 3, 128, ident);
    for (int n = 0; n < 256; ++n)
        for (int k = 0; k < NCOND; ++k) {
            t[OFF_WC0 + n * NCOND + k] = nf_code(SM_XYZ0_W, n, 63 + k, 171);
            t[OFF_WC3 + n * NCOND + k] = nf_code(SM_XYZ3_W, n, 63 + k, 427);
        }
    for (int n = 0; n < 128; ++n) {
        for (int f = 0; f < 4; ++f)
            for (int sc = 0; sc < 2; ++sc)
                for (int comp = 1; comp < 3; ++comp)
                    t[OFF_WCD + n * 16 + 4 * f + 2 * sc + (comp - 1)] = nf_code(SM_DIR0_W, n, 256 + 6 * f + 3 * sc + comp, 356);
        for (int k = 0; k < NEXPR; ++k) t[OFF_WCE + n * NEXPR + k] = nf_code(SM_DIR0_W, n, 280 + k, 356);
    }
    const int bias_ids[6] = {1, 3, 5, 7, 9, SM_FEAT_B};
    for (int l = 0; l < 6; ++l)
        for (int n = 0; n < 256; ++n) t[OFF_BIAS + 256 * l + n] = nf_code(bias_ids[l], 0, n, 256);
    for (int n = 0; n < 128; ++n) {
        t[OFF_BIAS + B_D0 + n] = nf_code(SM_DIR0_B, 0, n, 128);
        t[OFF_BIAS + B_D1 + n] = nf_code(17, 0, n, 128);
        t[OFF_BIAS + B_D2 + n] = nf_code(19, 0, n, 128);
    }
    t[OFF_BIAS + B_D0 + 128] = nf_code(SM_ALPHA_B, 0, 0, 1);
    for (int n = 0; n < 3; ++n) t[OFF_BIAS + B_RGB + n] = nf_code(SM_RGB_B, 0, n, 3);
}

static NfPackTable g_smaller_table;

extern "C" size_t nf_smaller_packed_floats(void) { return (size_t)nsm::PACKED; }
// 2076 floats are written; rounded up to whole KiB
extern "C" size_t nf_smaller_cond_floats(void) { return (size_t)((nsm::COND_FLOATS + 255) & ~255); }

// Host-side copy of the gather table (for layout tests without a GPU): code = tensor_id << 24 | offset.
extern "C" int nf_smaller_gather_table(uint32_t* out, size_t n) {
    if (!out || n != (size_t)nsm::PACKED) return NF_EINVAL;
    return nf_export_table(nf_smaller_table, out, n) == (long)n ? 0 : NF_EINVAL;
}

extern "C" int nf_smaller_pack(const float* const* params, float* packed, nf_stream_t stream) {
    return nf_pack_f32<nsm::NPARAMS, 8>(g_smaller_table, nf_smaller_table, params, packed, (int)nsm::PACKED, stream);
}

// =================================================================================================
// condition: per-call bias table
//   cond[L0]  = b0  + W0[:, 63:139] (expr*1/3) + W0[:, 139:171] latent                 (models.py:318-320)
//   cond[L3]  = b3  + W3[:, 63:171] [expr/3 ; latent]                                    (models.py:323)
//   cond[D0]  = bd0 + Wd0[:, 256 + 6f + 3sc + {1,2}] . {sin,cos}({near,far} 2^f)         (Quirk Q1)
//                   + Wd0[:, 280:356] (expr*1/3)                                         (models.py:330)
//   every other entry is the plain bias.  DIRS = false (pre-encoded inputs): the direction columns arrive with x, no Q1 fold.
// =================================================================================================
template <bool DIRS>
__global__ void __launch_bounds__(256) k_smaller_condition(const float* __restrict__ packed, const float* __restrict__ expr,
                                                           const float* __restrict__ latent, float near_z, float far_z,
                                                           float* __restrict__ cond) {
    using namespace nsm;
    __shared__ float cvec[NCOND];
    __shared__ float dvec[16];
    const int tid = threadIdx.x;
    if (tid < 76) cvec[tid] = nf_div(nf_mul(expr[tid], 1.0f), 3.0f);        // (expr * 1) / 3, a true division
    else if (tid < NCOND) cvec[tid] = latent[tid - 76];
    if (tid >= 128 && tid < 144) {
        const int k = tid - 128, f = k >> 2, sc = (k >> 1) & 1, comp = k & 1;
        const float a = nf_mul(comp ? far_z : near_z, exp2f((float)f));
        dvec[k] = DIRS ? (sc ? cosf(a) : sinf(a)) : 0.0f;
    }
    __syncthreads();
    const float* bias = packed + OFF_BIAS;
    for (int i = blockIdx.x * blockDim.x + tid; i < COND_FLOATS; i += gridDim.x * blockDim.x) {
        if (i >= B_CVEC) { cond[i] = i < B_DVEC ? cvec[i - B_CVEC] : dvec[i - B_DVEC]; continue; }
        float v = bias[i];
        if (i < B_L1 || (i >= B_L3 && i < B_L4)) {
            const int n = i < B_L1 ? i : i - B_L3;
            const float* w = packed + (i < B_L1 ? OFF_WC0 : OFF_WC3) + n * NCOND;
            float s = 0.0f;
            for (int k = 0; k < NCOND; ++k) s = fmaf(w[k], cvec[k], s);
            v += s;
        } else if (i >= B_D0 && i < B_D0 + 128) {
            float s = 0.0f;
            if (DIRS) {
                const float* w = packed + OFF_WCD + (i - B_D0) * 16;
                for (int k = 0; k < 16; ++k) s = fmaf(w[k], dvec[k], s);
            }
            const float* we = packed + OFF_WCE + (i - B_D0) * NEXPR;
            for (int k = 0; k < NEXPR; ++k) s = fmaf(we[k], cvec[k], s);
            v += s;
        }
        cond[i] = v;
    }
}

extern "C" int nf_smaller_condition(const float* packed, const float* expr76, const float* latent32, float near_z, float far_z,
                                    float* cond, nf_stream_t stream) {
    if (!packed || !expr76 || !latent32 || !cond) return NF_EINVAL;
    hipLaunchKernelGGL(k_smaller_condition<true>, dim3((nsm::COND_FLOATS + 255) / 256), dim3(256), 0, nf_s(stream), packed, expr76,
                       latent32, near_z, far_z, cond);
    NF_RETURN_LAUNCH();
}

// =================================================================================================
// forward
// =================================================================================================
// The network body from layers_xyz.0 to fc_rgb on the inference schedule, shared by the ray-input kernel and the pre-encoded one:
// every layer ends in nf_tail (raw accumulators to the slab tile by tile under the last chunk's MFMAs, the next layer's bias, first
// weights and first B fragment fetched), every layer starts with the bias as the C operand of its first MFMAs, the ReLU is applied
// where the slab is read.  NDIR register chunks of direction slots (1: (sin, cos)(rd_z 2^g), weights OFF_D0; 2: the 24 reference
// columns, weights OFF_D0E) follow layers_dir.0's 16 feat chunks.  Leaves rgb_raw in acc[t][0].xyz and sigma_raw in sigma_raw[t].
template <int NT, int NDIR>
__device__ __forceinline__ void nf_smaller_body(f32x4 (&acc)[NT][16], float (&sigma_raw)[NT], const f32x4 (&pe)[NT][4],
                                                const f32x4 (&dirf)[NT][NDIR], const NfW& Wi, const NfW& Ci, f32x4* act4, int lane) {
    using namespace nsm;
    constexpr unsigned D0 = (NDIR == 1 ? OFF_D0 : OFF_D0E) / 4;
    NfStream<NT> st;
    f32x4 bj[NT];
#define NF_PE_B(J_) do { _Pragma("unroll") for (int t = 0; t < NT; ++t) bj[t] = pe[t][J_]; } while (0)
    // ---- layers_xyz.0 : PE(64 slots) -> 256 ------------------------------------------------------------
    nf_load_bias<16>(st.bias, Ci, B_L0, lane);
    {
        f32x4 w[16];
        nf_load_w16<16>(w, Wi, OFF_L0 / 4, lane);
        NF_PE_B(0); nf_chunk<NT, 16, true>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L0 / 4 + 1 * 16 * 64, lane);
        NF_PE_B(1); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L0 / 4 + 2 * 16 * 64, lane);
        NF_PE_B(2); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L0 / 4 + 3 * 16 * 64, lane);
        NF_PE_B(3); nf_tail<NT, 16, 16, 16, 1>(acc, w, bj, st, Wi, OFF_L1 / 4, Ci, B_L1, act4, lane);
    }
    // ---- layers_xyz.1, .2 (ReLU of the previous layer on read) ------------------------------------------
    nf_seg_lds<NT, 16, true, true>(acc, st, Wi, OFF_L1 / 4, 16, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 16, 16, 16, 1>(acc, st.wb, bj, st, Wi, OFF_L2 / 4, Ci, B_L2, act4, lane);
    nf_seg_lds<NT, 16, true, true>(acc, st, Wi, OFF_L2 / 4, 16, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 16, 16, 16, 0>(acc, st.wb, bj, st, Wi, OFF_L3 / 4, Ci, B_L3, act4, lane);
    // ---- layers_xyz.3 : [PE | h] -> 256 (skip connection, M:323) ----------------------------------------
    NF_PE_B(0); nf_chunk<NT, 16, true>(acc, st.wa, bj, st.bias);
    nf_load_w16<16>(st.wa, Wi, OFF_L3 / 4 + 4 * 16 * 64, lane);            // the first slab chunk, three chunks ahead
    nf_read_b<NT>(st.b0, act4, lane, 0);
    {
        f32x4 w[16];
        nf_load_w16<16>(w, Wi, OFF_L3 / 4 + 1 * 16 * 64, lane);
        NF_PE_B(1); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L3 / 4 + 2 * 16 * 64, lane);
        NF_PE_B(2); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L3 / 4 + 3 * 16 * 64, lane);
        NF_PE_B(3); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);
    }
    nf_seg_lds<NT, 16, false, true>(acc, st, Wi, OFF_L3 / 4 + 4 * 16 * 64, 16, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 16, 16, 16, 1>(acc, st.wb, bj, st, Wi, OFF_L4 / 4, Ci, B_L4, act4, lane);
    // ---- layers_xyz.4 ------------------------------------------------------------------------------------
    nf_seg_lds<NT, 16, true, true>(acc, st, Wi, OFF_L4 / 4, 16, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 16, 16, 16, 1>(acc, st.wb, bj, st, Wi, OFF_FEAT / 4, Ci, B_FEAT, act4, lane);
    // ---- fc_feat (no activation, M:327: layers_dir.0 reads it as stored) ------------------------------------
    nf_seg_lds<NT, 16, true, true>(acc, st, Wi, OFF_FEAT / 4, 16, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 16, 16, 9, 1>(acc, st.wb, bj, st, Wi, D0, Ci, B_D0, act4, lane);
    // ---- layers_dir.0 : [feat | dir slots] -> 128; tile 8 row 0 = fc_alpha(feat) (M:328) ----------------------
    {
        f32x4 wd[16];
        nf_load_w16<9>(wd, Wi, D0 + 16 * 9 * 64, lane);                     // the first dir-slot chunk's weights, a layer ahead
        nf_seg_lds<NT, 9, true, false>(acc, st, Wi, D0, 16, act4, lane);
        nf_pending_b<NT, false>(bj, st);
        nf_chunk<NT, 9, false>(acc, st.wb, bj, st.bias);
        if (NDIR == 2) {
            nf_load_w16<9>(st.wb, Wi, D0 + 17 * 9 * 64, lane);
#pragma unroll
            for (int t = 0; t < NT; ++t) bj[t] = dirf[t][0];
            nf_chunk<NT, 9, false>(acc, wd, bj, st.bias);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) bj[t] = dirf[t][NDIR - 1];
        if constexpr (NDIR == 2) nf_tail<NT, 9, 8, 8, 1>(acc, st.wb, bj, st, Wi, OFF_D1 / 4, Ci, B_D1, act4, lane);
        else nf_tail<NT, 9, 8, 8, 1>(acc, wd, bj, st, Wi, OFF_D1 / 4, Ci, B_D1, act4, lane);
#pragma unroll
        for (int t = 0; t < NT; ++t) sigma_raw[t] = acc[t][8].x;
    }
    // ---- layers_dir.1, .2 -----------------------------------------------------------------------------------
    nf_seg_lds<NT, 8, true, true>(acc, st, Wi, OFF_D1 / 4, 8, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 8, 8, 8, 1>(acc, st.wb, bj, st, Wi, OFF_D2 / 4, Ci, B_D2, act4, lane);
    nf_seg_lds<NT, 8, true, true>(acc, st, Wi, OFF_D2 / 4, 8, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 8, 8, 1, 1>(acc, st.wb, bj, st, Wi, OFF_RGB / 4, Ci, B_RGB, act4, lane);
#undef NF_PE_B
    // ---- fc_rgb -------------------------------------------------------------------------------------------
    nf_seg_lds<NT, 1, true, true>(acc, st, Wi, OFF_RGB / 4, 8, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_chunk<NT, 1, false>(acc, st.wb, bj, st.bias);
}

// inputs of one wave: pts = ro + rd*z (T:78), PE fragments, dir fragment
template <int NT>
__device__ __forceinline__ void nf_smaller_inputs(f32x4 (&pe)[NT][4], f32x4 (&dirf)[NT][1], int64_t p0, int64_t n_points, int S, int lane,
                                                  const float* __restrict__ ro, const float* __restrict__ rd,
                                                  const float* __restrict__ rd_view, const float* __restrict__ z) {
    const int g = lane >> 4, c = lane & 15;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int64_t p = p0 + 16 * t + c;
        if (p >= n_points) p = n_points - 1;
        const int64_t ray = p / S;
        const float zz = z[p];
        const float dx = rd[ray * 3 + 0], dy = rd[ray * 3 + 1], dz = rd[ray * 3 + 2];
        const float px = nf_add(ro[ray * 3 + 0], nf_mul(dx, zz));
        const float py = nf_add(ro[ray * 3 + 1], nf_mul(dy, zz));
        const float pz = nf_add(ro[ray * 3 + 2], nf_mul(dz, zz));
        nf_encode_point(px, py, pz, g, pe[t]);
        float s, cs;
        nf_sincos(nf_mul(rd_view[ray * 3 + 2], (float)(1 << g)), &s, &cs);   // Quirk Q1: "direction" = (rd_z, near, far)
        dirf[t][0] = (f32x4){s, cs, 0.0f, 0.0f};
    }
}

template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_smaller_mlp_fwd(const float* __restrict__ packed, const float* __restrict__ cond_, const float* __restrict__ ro,
                  const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z,
                  int64_t n_points, int S, float* __restrict__ raw) {
    using namespace nsm;
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15;
    f32x4* act4 = lds + wave * (16 * NT * 64);
    typedef __attribute__((address_space(1))) f32x4 nf_gf32x4;
    nf_gf32x4* raw_v = (nf_gf32x4*)raw;               // the output pointer and the grid stride live in VGPRs (see the epilogue)
    asm volatile("" : "+v"(raw_v));
    int stride_v = (int)gridDim.x;
    asm volatile("" : "+v"(stride_v));
    // persistent form, as k_paper_mlp_fwd: one workgroup per CU walks the point blocks with the grid's stride
#pragma unroll 1
    for (int64_t blk = blockIdx.x;; blk += __builtin_amdgcn_readfirstlane(stride_v)) {
    const int64_t p0 = (blk * NF_MLP_WAVES + wave) * (16 * NT);
    if (p0 >= n_points) break;                        // wave-uniform; no barriers anywhere below
    int opaque0 = 0;                                  // per-block opaque zero: the weight / bias loads must stay where the layers issue them
    asm volatile("" : "+s"(opaque0));
    const float* W = packed + opaque0;
    const float* cond = cond_ + opaque0;
    f32x4 pe[NT][4];
    f32x4 dirf[NT][1];
    nf_smaller_inputs<NT>(pe, dirf, p0, n_points, S, lane, ro, rd, rd_view, z);
    f32x4 acc[NT][16];
    float sigma_raw[NT];
    const NfW Wi = nf_w_image(W, PACKED), Ci = nf_w_image(cond, COND_FLOATS);
    nf_smaller_body<NT, 1>(acc, sigma_raw, pe, dirf, Wi, Ci, act4, lane);
    // (the store predicate, the output pointer and the grid stride are re-derived from opaque VGPR copies: as loop invariants of the
    // persistent block loop they would otherwise be held in scalar registers the K loops need)
    int lane_o = lane;
    asm volatile("" : "+v"(lane_o));
    if ((lane_o >> 4) == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int64_t p = p0 + 16 * t + c;
            if (p < n_points)
                raw_v[p] = (f32x4){acc[t][0].x, acc[t][0].y, acc[t][0].z, sigma_raw[t]};
        }
    }
    }
}

// ConditionalBlendshapePaperSmallerNeRFModel.forward on PRE-ENCODED inputs (M:313-338 as run_network calls it, T:9-33):
// x (P, 87) = [PE10(xyz) (63) | PE4(dirs) (24)] -> (P, 4).  Inference only; the hot path never materialises x.  Same body, inputs
// from x87, layers_dir.0 with its 24 direction columns as two register chunks, bias table without the direction fold.
template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_smaller_mlp_fwd_encoded(const float* __restrict__ packed, const float* __restrict__ cond, const float* __restrict__ x87,
                          int64_t n_points, float* __restrict__ out) {
    using namespace nsm;
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int64_t p0 = ((int64_t)blockIdx.x * NF_MLP_WAVES + wave) * (16 * NT);
    if (p0 >= n_points) return;
    f32x4* act4 = lds + wave * (16 * NT * 64);
    f32x4 pe[NT][4];
    f32x4 dirf[NT][2];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int64_t p = p0 + 16 * t + c;
        if (p >= n_points) p = n_points - 1;
        const float* row = x87 + p * 87;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = nfl::pe_slot_to_col(16 * j + 4 * g + r);
                v[r] = col >= 0 ? row[col] : 0.0f;
            }
            pe[t][j] = (f32x4){v[0], v[1], v[2], v[3]};
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = 16 * j + 4 * g + r;
                v[r] = s < 24 ? row[63 + s] : 0.0f;
            }
            dirf[t][j] = (f32x4){v[0], v[1], v[2], v[3]};
        }
    }
    f32x4 acc[NT][16];
    float sigma_raw[NT];
    const NfW Wi = nf_w_image(packed, PACKED), Ci = nf_w_image(cond, COND_FLOATS);
    nf_smaller_body<NT, 2>(acc, sigma_raw, pe, dirf, Wi, Ci, act4, lane);
    if (g == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int64_t p = p0 + 16 * t + c;
            if (p < n_points) reinterpret_cast<f32x4*>(out)[p] = (f32x4){acc[t][0].x, acc[t][0].y, acc[t][0].z, sigma_raw[t]};
        }
    }
}

// x87: (n_points, 87) pre-encoded inputs; cond: scratch of nf_smaller_cond_floats() floats; out: (n_points, 4).
extern "C" int nf_smaller_forward_encoded(const float* packed, const float* x87, const float* expr76, const float* latent32,
                                          int64_t n_points, float* cond, float* out, nf_stream_t stream) {
    if (n_points == 0) return 0;                           // nothing to do (empty tensors have NULL data pointers)
    if (!packed || !x87 || !expr76 || !latent32 || !cond || !out || n_points < 0) return NF_EINVAL;
    hipLaunchKernelGGL(k_smaller_condition<false>, dim3((nsm::COND_FLOATS + 255) / 256), dim3(256), 0, nf_s(stream), packed, expr76,
                       latent32, 0.0f, 0.0f, cond);
    constexpr int NT = NF_MLP_NT;
    const int64_t per_block = (int64_t)NF_MLP_WAVES * 16 * NT;
    const int64_t grid = (n_points + per_block - 1) / per_block;
    if (grid > 0x7fffffff) return NF_EINVAL;
    hipLaunchKernelGGL((k_smaller_mlp_fwd_encoded<NT>), dim3((unsigned)grid), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream), packed, cond, x87,
                       n_points, out);
    NF_RETURN_LAUNCH();
}

// Training forward (exact f32): the same arithmetic as k_smaller_mlp_fwd, plus everything the backward needs in `saved` (layout
// nsm::S_*): every layer output as row-major [n][width] matrices for the weight-gradient GEMMs -- copied out of the wave's LDS slab
// as whole 128-byte lines from inside the NEXT layer's K loop -- and the ReLU bit masks the dX chain applies (k_paper_mlp_fwd_save,
// nf_mlp.hip, is the template).
template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_smaller_mlp_fwd_save(const float* __restrict__ packed, const float* __restrict__ cond, const float* __restrict__ ro,
                       const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z,
                       int64_t n_points, int S, float* __restrict__ raw, float* __restrict__ saved) {
    using namespace nsm;
    static_assert(NT == 2, "the copy schedule below is written for 32-point slabs");
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int64_t p0 = ((int64_t)blockIdx.x * NF_MLP_WAVES + wave) * (16 * NT);
    if (p0 >= n_points) return;                       // wave-uniform; no barriers anywhere below
    f32x4* act4 = lds + wave * (16 * NT * 64);
    const int64_t n = n_points;
    auto sec = [&](int s, int width) { return nf_slab_copy(saved, s, width, p0, n); };

    f32x4 pe[NT][4];
    f32x4 dirf[NT][1];
    nf_smaller_inputs<NT>(pe, dirf, p0, n_points, S, lane, ro, rd, rd_view, z);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int64_t p = p0 + 16 * t + c;
        // dir slots: 64 B per point, the 16 points of a tile are one contiguous KiB
        if (p < n_points) *reinterpret_cast<f32x4*>(saved + S_DIRF * n_points + p * 16 + 4 * g) = dirf[t][0];
#pragma unroll
        for (int j = 0; j < 4; ++j) act4[nf_act_idx4(16 * t + c, 4 * j + g)] = pe[t][j];       // PE slots 16 j + 4 g .. + 3
    }
    {   // PE rows (64 slots = 256 B per point): four rows per instruction, before layers_xyz.0's output takes the slab
        const NfSlabCopy cp = sec(S_PE, 64);
#pragma unroll
        for (int k = 0; k < 16 * NT / 4; ++k) nf_copy_rows<16>(act4, cp, k, lane);
    }

    f32x4 acc[NT][16];
    uint64_t m64[NT];
    NfStream<NT> st;
    f32x4 bj[NT];
    const NfW Wi = nf_w_image(packed, PACKED), Ci = nf_w_image(cond, COND_FLOATS);
#define NF_PE_B(J_) do { _Pragma("unroll") for (int t = 0; t < NT; ++t) bj[t] = pe[t][J_]; } while (0)
    // the last chunk's fragment (+ its mask bits), then the finished mask words of layer MASKL_ (the layer whose output was just consumed)
#define NF_SM_PENDING(RELU_, MASKL_, NCH_)                                                           \
    do {                                                                                            \
        nf_pending_b<NT, RELU_>(bj, st);                                                            \
        if ((MASKL_) >= 0) {                                                                        \
            nf_mask_bits<NT>(m64, st.bp, (NCH_) - 2);                                               \
            nf_mask_bits<NT>(m64, bj, (NCH_) - 1);                                                  \
            _Pragma("unroll") for (int t = 0; t < NT; ++t)                                          \
                if (p0 + 16 * t < n)                                                                \
                    *nf_mask_ptr<S_MASK>(saved, n, (MASKL_) >= 0 ? (MASKL_) : 0, (p0 >> 4) + t, lane) = make_uint2((uint32_t)m64[t], (uint32_t)(m64[t] >> 32)); \
        }                                                                                           \
    } while (0)
    // one 256-wide layer from the slab: the slab = section SEC_ (ReLU layer MASKL_, or -1: as stored) is copied out and consumed
#define NF_SM_LAYER256(OFF_, FIRST_, SEC_, MASKL_, OFF_NEXT_, B_NEXT_, NO_NEXT_, NEXT_B_)                                 \
    do {                                                                                                                   \
        NfCopyH<64, 4, ((MASKL_) >= 0)> cs{act4, sec(SEC_, 256), lane, 8, {}};                                             \
        cs.prime();                                                                                                        \
        _Pragma("unroll") for (int t = 0; t < NT; ++t) m64[t] = 0;                                                         \
        nf_seg_lds<NT, 16, FIRST_, ((MASKL_) >= 0), ((MASKL_) >= 0)>(acc, st, Wi, OFF_, 16, act4, lane, cs, m64);          \
        NF_SM_PENDING(((MASKL_) >= 0), MASKL_, 16);                                                                        \
        nf_tail<NT, 16, 16, NO_NEXT_, NEXT_B_>(acc, st.wb, bj, st, Wi, OFF_NEXT_, Ci, B_NEXT_, act4, lane);               \
    } while (0)
    // ---- layers_xyz.0 : PE(64 slots) -> 256 ------------------------------------------------------------
    nf_load_bias<16>(st.bias, Ci, B_L0, lane);
    {
        f32x4 w[16];
        nf_load_w16<16>(w, Wi, OFF_L0 / 4, lane);
        NF_PE_B(0); nf_chunk<NT, 16, true>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L0 / 4 + 1 * 16 * 64, lane);
        NF_PE_B(1); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L0 / 4 + 2 * 16 * 64, lane);
        NF_PE_B(2); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L0 / 4 + 3 * 16 * 64, lane);
        NF_PE_B(3); nf_tail<NT, 16, 16, 16, 1>(acc, w, bj, st, Wi, OFF_L1 / 4, Ci, B_L1, act4, lane);
    }
    // ---- layers_xyz.1, .2 (each K loop also streams the layer output it consumes to `saved`) -------------
    NF_SM_LAYER256(OFF_L1 / 4, true, S_H0, 0, OFF_L2 / 4, B_L2, 16, 1);
    NF_SM_LAYER256(OFF_L2 / 4, true, S_H1, 1, OFF_L3 / 4, B_L3, 16, 0);
    // ---- layers_xyz.3 : [PE | h] -> 256 (skip connection, M:323) ------------------------------------
    NF_PE_B(0); nf_chunk<NT, 16, true>(acc, st.wa, bj, st.bias);
    nf_load_w16<16>(st.wa, Wi, OFF_L3 / 4 + 4 * 16 * 64, lane);            // the first slab chunk, three chunks ahead
    nf_read_b<NT>(st.b0, act4, lane, 0);
    {
        f32x4 w[16];
        nf_load_w16<16>(w, Wi, OFF_L3 / 4 + 1 * 16 * 64, lane);
        NF_PE_B(1); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L3 / 4 + 2 * 16 * 64, lane);
        NF_PE_B(2); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L3 / 4 + 3 * 16 * 64, lane);
        NF_PE_B(3); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);
    }
    NF_SM_LAYER256(OFF_L3 / 4 + 4 * 16 * 64, false, S_H2, 2, OFF_L4 / 4, B_L4, 16, 1);
    // ---- layers_xyz.4, fc_feat (no activation, M:327) -----------------------------------------------
    NF_SM_LAYER256(OFF_L4 / 4, true, S_H3, 3, OFF_FEAT / 4, B_FEAT, 16, 1);
    NF_SM_LAYER256(OFF_FEAT / 4, true, S_H4, 4, OFF_D0 / 4, B_D0, 9, 1);
    // ---- layers_dir.0 : [feat | dir slots] -> 128; tile 8 row 0 = fc_alpha(feat) (M:328) ------------------
    float sigma_raw[NT];
    {
        f32x4 wd[16];
        nf_load_w16<9>(wd, Wi, OFF_D0 / 4 + 16 * 9 * 64, lane);             // the dir-slot chunk's weights, a layer ahead
        NfCopyH<64, 4, false> cs{act4, sec(S_FEAT, 256), lane, 8, {}};
        cs.prime();
        nf_seg_lds<NT, 9, true, false, false>(acc, st, Wi, OFF_D0 / 4, 16, act4, lane, cs, m64);
        NF_SM_PENDING(false, -1, 16);
        nf_chunk<NT, 9, false>(acc, st.wb, bj, st.bias);
#pragma unroll
        for (int t = 0; t < NT; ++t) bj[t] = dirf[t][0];
        nf_tail<NT, 9, 8, 8, 1>(acc, wd, bj, st, Wi, OFF_D1 / 4, Ci, B_D1, act4, lane);
#pragma unroll
        for (int t = 0; t < NT; ++t) sigma_raw[t] = acc[t][8].x;
    }
    // ---- layers_dir.1, .2, fc_rgb (128-wide rows: two per copy instruction) --------------------------------
#define NF_SM_LAYER128(OFF_, NO_, SEC_, MASKL_)                                                                           \
    NfCopyH<32, 4, true> cs{act4, sec(SEC_, 128), lane, 4, {}};                                                            \
    cs.prime();                                                                                                            \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) m64[t] = 0;                                                             \
    nf_seg_lds<NT, NO_, true, true, true>(acc, st, Wi, OFF_, 8, act4, lane, cs, m64);                                      \
    NF_SM_PENDING(true, MASKL_, 8)
    {
        NF_SM_LAYER128(OFF_D1 / 4, 8, S_D0, 5);
        nf_tail<NT, 8, 8, 8, 1>(acc, st.wb, bj, st, Wi, OFF_D2 / 4, Ci, B_D2, act4, lane);
    }
    {
        NF_SM_LAYER128(OFF_D2 / 4, 8, S_D1, 6);
        nf_tail<NT, 8, 8, 1, 1>(acc, st.wb, bj, st, Wi, OFF_RGB / 4, Ci, B_RGB, act4, lane);
    }
    {
        NF_SM_LAYER128(OFF_RGB / 4, 1, S_D2, 7);
        nf_chunk<NT, 1, false>(acc, st.wb, bj, st.bias);
    }
#undef NF_SM_LAYER128
#undef NF_SM_LAYER256
#undef NF_SM_PENDING
#undef NF_PE_B
    if (g == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int64_t p = p0 + 16 * t + c;
            if (p < n_points)
                reinterpret_cast<f32x4*>(raw)[p] = (f32x4){acc[t][0].x, acc[t][0].y, acc[t][0].z, sigma_raw[t]};
        }
    }
}

static int nf_smaller_launch_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                 const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream) {
    constexpr int NT = NF_MLP_NT;
    static_assert(NF_MLP_WAVES * 16 * NT == 128, "nf_mlp_fwd_launch sizes the grid for 128 points per workgroup");
    const float* rdv = rd_view ? rd_view : rd;
    return nf_mlp_fwd_launch(saved ? NF_FWD_TRAIN_F32 : NF_FWD_INFER, packed, cond, ro, rd, z, raw, saved, n_rays, n_samples,
                             [&](int64_t n_points, unsigned grid) {
        if (saved)
            hipLaunchKernelGGL((k_smaller_mlp_fwd_save<NT>), dim3(grid), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream), packed, cond, ro, rd, rdv, z,
                               n_points, n_samples, raw, saved);
        else                                                    // inference: a persistent grid, at most one workgroup per CU
            hipLaunchKernelGGL((k_smaller_mlp_fwd<NT>), dim3((unsigned)(grid < nf_cu_count() ? grid : nf_cu_count())), dim3(64 * NF_MLP_WAVES), 0,
                               nf_s(stream), packed, cond, ro, rd, rdv, z, n_points, n_samples, raw);
    });
}

extern "C" int nf_smaller_mlp_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                  const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream) {
    return nf_smaller_launch_fwd(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, nullptr, stream);
}

// + one point tile of mask words per ReLU layer: the masks are kept per 16-point tile, ceil(n / 16) of them per layer
extern "C" size_t nf_smaller_saved_floats(int64_t n_points) {
    return (size_t)nsm::SAVED_PER_POINT * (size_t)((n_points + 31) & ~(int64_t)31) + nsm::N_RELU * 128;
}

// Training forward: also fills `saved` (nf_smaller_saved_floats(n_points) floats), which nf_smaller_mlp_bwd reads.
extern "C" int nf_smaller_mlp_fwd_train(const float* packed, const float* cond, const float* ro, const float* rd,
                                        const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,
                                        float* saved, nf_stream_t stream) {
    if (!saved) return NF_EINVAL;
    return nf_smaller_launch_fwd(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, saved, stream);
}
