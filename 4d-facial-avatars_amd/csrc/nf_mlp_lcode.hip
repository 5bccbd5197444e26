// Second model family: ConditionalBlendshapeLearnableCodeNeRFModel (reference nerf/models.py:529-636) as every NeRFace
// config instantiates it (num_layers 4, hidden 256, no skip, 10/4 encoding functions, include_input_dir False):
//   x = layer1([PE(63) | expr/3 (76) | latent (32)])          (no activation)
//   3 x relu(layers_xyz.i(x));  feat = relu(fc_feat(x));  sigma = fc_alpha(x)   (reads x, not feat)
//   relu(layers_dir.0([feat | PE4(dir) (24)])) -> rgb = fc_rgb
// Inference forward, exact-f32 MFMA, same building blocks / folding rules as the paper model (nf_mlp.hip).
#include <vector>
#include <mutex>
#include "nf_mlp_lcode_net.h"

// gather table of the exact-f32 image for a class of geometry `ge` (nf_mlp_lcode_layout.h)
void nf_lcode_build_table(std::vector<uint32_t>& t, const NfLcodeGeom& ge) {
    using namespace nlc;
    const int* id = ge.id;
    t.assign(PACKED, NF_ZERO_CODE);
    auto fill = [&](int off, int nk, int no_tiles, int tensor, int n_out, int n_cols, auto col_of) {
        nf_fill_frag(t, off, nk, no_tiles, [&](int slot, int n) {
            const int col = col_of(slot);
            return n < n_out && col >= 0 ? nf_code(tensor, n, col, n_cols) : NF_ZERO_CODE;
        });
    };
    auto ident = [](int s) { return s; };
    fill(OFF_L1, 4, 16, id[0], 256, ge.ld1, [](int s) { return nfl::pe_slot_to_col(s); });
    fill(OFF_X0, 16, 16, id[2], 256, 256, ident);
    fill(OFF_X1, 16, 16, id[4], 256, 256, ident);
    fill(OFF_X2, 16, 16, id[6], 256, 256, ident);
    fill(OFF_ALPHA, 16, 1, id[10], 1, 256, ident);
    fill(OFF_FEAT, 16, 16, id[14], 256, 256, ident);
    fill(OFF_DIR, 17, 8, id[8], 128, 280, [](int s) {
        if (s < 256) return s;
        const int g = ((s - 256) >> 2) & 3, r = (s - 256) & 3;
        return r < 2 ? 256 + 6 * g + 3 * r : -1;
    });
    fill(OFF_RGB, 8, 1, id[12], 3, 128, ident);
    fill(OFF_DIRE, 18, 8, id[8], 128, 280, [](int s) { return s < 280 ? s : -1; });
    for (int n = 0; n < 256; ++n)
        for (int k = 0; k < ge.n_cond; ++k) t[OFF_WC1 + n * 108 + k] = nf_code(id[0], n, 63 + k, ge.ld1);
    for (int n = 0; n < 128; ++n)
        for (int f = 0; f < 4; ++f)
            for (int sc = 0; sc < 2; ++sc)
                for (int comp = 1; comp < 3; ++comp) t[OFF_WCD + n * 16 + 4 * f + 2 * sc + (comp - 1)] = nf_code(id[8], n, 256 + 6 * f + 3 * sc + comp, 280);
    const int b256[5] = {1, 3, 5, 7, 15};          // layer1, layers_xyz.0..2, fc_feat biases
    for (int l = 0; l < 5; ++l)
        for (int n = 0; n < 256; ++n) t[OFF_BIAS + 256 * l + n] = nf_code(id[b256[l]], 0, n, 256);
    t[OFF_BIAS + B_ALPHA] = nf_code(id[11], 0, 0, 1);
    for (int n = 0; n < 128; ++n) t[OFF_BIAS + B_DIR + n] = nf_code(id[9], 0, n, 128);
    for (int n = 0; n < 3; ++n) t[OFF_BIAS + B_RGB + n] = nf_code(id[13], 0, n, 3);
}

static void nf_lcode_table(std::vector<uint32_t>& t) { nf_lcode_build_table(t, NF_LCODE_GEOM); }

static NfPackTable g_lcode_table;

extern "C" size_t nf_lcode_packed_floats(void) { return (size_t)nlc::PACKED; }
// padded to 10 KiB: the split-bf16 kernel stages the table into LDS with ten 1-KiB DMA pieces
extern "C" size_t nf_lcode_cond_floats(void) { return 2560; }

extern "C" int nf_lcode_pack(const float* const* params, float* packed, nf_stream_t stream) {
    return nf_pack_f32<nlc::NPARAMS, 4>(g_lcode_table, nf_lcode_table, params, packed, (int)nlc::PACKED, stream);
}

__global__ void __launch_bounds__(256) k_lcode_condition(const float* __restrict__ packed, const float* __restrict__ expr,
                                                         const float* __restrict__ latent, float near_z, float far_z,
                                                         float* __restrict__ cond) {
    __shared__ float cvec[108];
    __shared__ float dvec[16];
    const int tid = threadIdx.x;
    if (tid < 76) cvec[tid] = nf_div(nf_mul(expr[tid], 1.0f), 3.0f);        // (expr * 1) / 3, a true division
    else if (tid < 108) cvec[tid] = latent[tid - 76];
    if (tid >= 128 && tid < 144) dvec[tid - 128] = nf_lcode_dvec(tid - 128, near_z, far_z);
    __syncthreads();
    nf_lcode_bias_table<108, false>(packed, cvec, dvec, cond);
}

extern "C" int nf_lcode_condition(const float* packed, const float* expr76, const float* latent32, float near_z, float far_z,
                                  float* cond, nf_stream_t stream) {
    if (!packed || !expr76 || !latent32 || !cond) return NF_EINVAL;
    hipLaunchKernelGGL(k_lcode_condition, dim3((nlc::COND_FLOATS + 255) / 256), dim3(256), 0, nf_s(stream), packed, expr76, latent32,
                       near_z, far_z, cond);
    NF_RETURN_LAUNCH();
}

template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_lcode_mlp_fwd(const float* __restrict__ packed, const float* __restrict__ cond, const float* __restrict__ ro,
                const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z, int64_t n_points, int S,
                float* __restrict__ raw) {
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p0 = ((int64_t)blockIdx.x * NF_MLP_WAVES + wave) * (16 * NT);
    if (p0 >= n_points) return;                       // wave-uniform; no barriers anywhere below
    f32x4* act4 = lds + wave * (16 * NT * 64);
    f32x4 pe[NT][4];
    f32x4 dirf[NT][1];
    nf_net_inputs<NT>(pe, dirf, p0, n_points, S, lane, ro, rd, rd_view, z);
    f32x4 acc[NT][16];
    float sigma_raw[NT];
    const NfW Wi = nf_w_image(packed, nlc::PACKED), Ci = nf_w_image(cond, nlc::COND_FLOATS);
    nf_lcode_net_body<NT, 1>(acc, sigma_raw, pe, dirf, Wi, Ci, act4, lane);
    nf_net_store_raw<NT>(acc, sigma_raw, p0, n_points, lane, raw);
}

// ConditionalBlendshapeLearnableCodeNeRFModel.forward on PRE-ENCODED inputs (reference nerf/models.py:590-636 as called by run_network,
// nerf/train_utils.py:9-33): x (P, 87) = [PE10(xyz) (63) | PE4(dirs) (24)] -> (P, 4).  Inference only; the hot path
// (run_one_iter_of_nerf) never materialises x and uses nf_lcode_mlp_fwd.  Same body as k_lcode_mlp_fwd, inputs from x87, layers_dir.0
// with its 24 direction columns as two register chunks (weights OFF_DIRE), bias table without the direction fold.
__global__ void __launch_bounds__(256) k_lcode_condition_encoded(const float* __restrict__ packed, const float* __restrict__ expr,
                                                                 const float* __restrict__ latent, float* __restrict__ cond) {
    __shared__ float cvec[108];
    const int tid = threadIdx.x;
    if (tid < 76) cvec[tid] = nf_div(nf_mul(expr[tid], 1.0f), 3.0f);
    else if (tid < 108) cvec[tid] = latent[tid - 76];
    __syncthreads();
    nf_lcode_bias_table<108, true>(packed, cvec, nullptr, cond);
}

template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_lcode_mlp_fwd_encoded(const float* __restrict__ packed, const float* __restrict__ cond, const float* __restrict__ x87, int64_t n_points,
                        float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p0 = ((int64_t)blockIdx.x * NF_MLP_WAVES + wave) * (16 * NT);
    if (p0 >= n_points) return;
    f32x4* act4 = lds + wave * (16 * NT * 64);
    f32x4 pe[NT][4];
    f32x4 dirf[NT][2];
    nf_net_inputs_encoded<NT>(pe, dirf, p0, n_points, lane, x87);
    f32x4 acc[NT][16];
    float sigma_raw[NT];
    const NfW Wi = nf_w_image(packed, nlc::PACKED), Ci = nf_w_image(cond, nlc::COND_FLOATS);
    nf_lcode_net_body<NT, 2>(acc, sigma_raw, pe, dirf, Wi, Ci, act4, lane);
    nf_net_store_raw<NT>(acc, sigma_raw, p0, n_points, lane, out);
}

// x87: (n_points, 87) pre-encoded inputs; cond: scratch of nf_lcode_cond_floats() floats; out: (n_points, 4).
extern "C" int nf_lcode_forward_encoded(const float* packed, const float* x87, const float* expr76, const float* latent32,
                                        int64_t n_points, float* cond, float* out, nf_stream_t stream) {
    if (n_points == 0) return 0;                           // nothing to do (empty tensors have NULL data pointers)
    if (!packed || !x87 || !expr76 || !latent32 || !cond || !out || n_points < 0) return NF_EINVAL;
    hipLaunchKernelGGL(k_lcode_condition_encoded, dim3((nlc::COND_FLOATS + 255) / 256), dim3(256), 0, nf_s(stream), packed, expr76,
                       latent32, cond);
    return nf_lcode_launch_fwd_encoded(packed, cond, x87, n_points, out, stream);
}

// k_lcode_mlp_fwd_encoded on a bias table that is already filled (also the classes of nf_mlp_bshape.hip / nf_mlp_cbshape.hip)
int nf_lcode_launch_fwd_encoded(const float* packed, const float* cond, const float* x87, int64_t n_points, float* out, nf_stream_t stream) {
    constexpr int NT = NF_MLP_NT;
    const int64_t per_block = (int64_t)NF_MLP_WAVES * 16 * NT;
    const int64_t grid = (n_points + per_block - 1) / per_block;
    if (grid > 0x7fffffff) return NF_EINVAL;
    hipLaunchKernelGGL((k_lcode_mlp_fwd_encoded<NT>), dim3((unsigned)grid), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream), packed, cond, x87,
                       n_points, out);
    NF_RETURN_LAUNCH();
}

// Training forward (exact f32): the same arithmetic plus `saved` (layout nlc::S_*) -- every layer output as whole rows out of the
// wave's LDS slab from inside the next layer's K loop, ReLU bit masks beside them (nf_mlp_dev.h, nf_mlp_stream.h; the same form as
// the paper model's nf_paper_net_body_save, nf_mlp_paper_net.h).
template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_lcode_mlp_fwd_save(const float* __restrict__ packed, const float* __restrict__ cond, const float* __restrict__ ro,
                     const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z, int64_t n_points, int S,
                     float* __restrict__ raw, float* __restrict__ saved) {
    using namespace nlc;
    using Net = NfLcodeNet;
    static_assert(NT == 2, "the copy schedule below is written for 32-point slabs");
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int64_t p0 = ((int64_t)blockIdx.x * NF_MLP_WAVES + wave) * (16 * NT);
    if (p0 >= n_points) return;
    f32x4* act4 = lds + wave * (16 * NT * 64);
    const int64_t n = n_points;
    auto sec = [&](int s_, int width) { return nf_slab_copy(saved, s_, width, p0, n); };
    f32x4 pe[NT][4];
    f32x4 dirf[NT][1];
    nf_net_inputs<NT>(pe, dirf, p0, n_points, S, lane, ro, rd, rd_view, z);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int64_t p = p0 + 16 * t + c;
        if (p < n) *reinterpret_cast<f32x4*>(saved + S_DIRF * n + p * 16 + 4 * g) = dirf[t][0];
#pragma unroll
        for (int j = 0; j < 4; ++j) act4[nf_act_idx4(16 * t + c, 4 * j + g)] = pe[t][j];
    }
    {
        const NfSlabCopy cp = sec(S_PE, 64);
#pragma unroll
        for (int k = 0; k < 16 * NT / 4; ++k) nf_copy_rows<16>(act4, cp, k, lane);
    }
    // Layer-streamed like k_paper_mlp_fwd_save (nf_mlp.hip) and this family's inference kernel above: bias as the C operand, the layer
    // boundary under the last chunk's MFMAs (raw accumulators to the slab), the next layer prefetched; what the backward needs is produced
    // where the slab is READ -- the loop that consumes a layer's output applies the ReLU to its B fragments, collects their [x > 0] bits
    // and carries the copy of the slab to `saved`.  layers_xyz.2's output is read twice (fc_alpha, fc_feat): copied and masked under fc_feat.
    f32x4 acc[NT][16];
    uint64_t m64[NT];
    NfStream<NT> st;
    f32x4 bj[NT];
    float sigma_raw[NT];
    const NfW Wi = nf_w_image(packed, PACKED), Ci = nf_w_image(cond, COND_FLOATS);
    // ---- layer1 : PE(64 slots) -> 256, no activation (M:609) ---------------------------------------------------------
    NF_NET_PE_LAYER(B_L1, OFF_L1, OFF_X0, B_X0);
    // ---- layers_xyz.0 (reads layer1's output as stored), .1, .2 ---------------------------------------------------------
    NF_NET_SAVE_LAYER256(OFF_X0 / 4, true, S_L1, -1, OFF_X1 / 4, B_X1, 16, 1);
    NF_NET_SAVE_LAYER256(OFF_X1 / 4, true, S_X0, 0, OFF_X2 / 4, B_X2, 16, 1);
    NF_NET_SAVE_LAYER256(OFF_X2 / 4, true, S_X1, 1, OFF_ALPHA / 4, B_ALPHA, 1, 1);
    // ---- fc_alpha(x2): one tile, stores nothing (the slab stays for fc_feat), copies nothing -------------------------------
    nf_seg_lds<NT, 1, true, true>(acc, st, Wi, OFF_ALPHA / 4, 16, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 1, 0, 16, 1>(acc, st.wb, bj, st, Wi, OFF_FEAT / 4, Ci, B_FEAT, act4, lane);
#pragma unroll
    for (int t = 0; t < NT; ++t) sigma_raw[t] = acc[t][0].x;
    // ---- feat = relu(fc_feat(x2)): x2 is copied and its mask collected here ---------------------------------------------
    NF_NET_SAVE_LAYER256(OFF_FEAT / 4, true, S_X2, 2, OFF_DIR / 4, B_DIR, 8, 1);
    // ---- layers_dir.0 : [feat | dir slots] -> 128 ---------------------------------------------------------------------------
    {
        f32x4 wd[16];
        nf_load_w16<8>(wd, Wi, OFF_DIR / 4 + 16 * 8 * 64, lane);             // the dir-slot chunk's weights, a layer ahead
        NfCopyH<64, 4, true> cs{act4, sec(S_FEAT, 256), lane, 8, {}};
        cs.prime();
#pragma unroll
        for (int t = 0; t < NT; ++t) m64[t] = 0;
        nf_seg_lds<NT, 8, true, true, true>(acc, st, Wi, OFF_DIR / 4, 16, act4, lane, cs, m64);
        NF_NET_SAVE_PENDING(true, 3, 16);
        nf_chunk<NT, 8, false>(acc, st.wb, bj, st.bias);
#pragma unroll
        for (int t = 0; t < NT; ++t) bj[t] = dirf[t][0];
        nf_tail<NT, 8, 8, 1, 1>(acc, wd, bj, st, Wi, OFF_RGB / 4, Ci, B_RGB, act4, lane);
    }
    // ---- fc_rgb (128-wide rows: two per copy instruction) ---------------------------------------------------------------------
    {
        NfCopyH<32, 4, true> cs{act4, sec(S_DIR, 128), lane, 4, {}};
        cs.prime();
#pragma unroll
        for (int t = 0; t < NT; ++t) m64[t] = 0;
        nf_seg_lds<NT, 1, true, true, true>(acc, st, Wi, OFF_RGB / 4, 8, act4, lane, cs, m64);
        NF_NET_SAVE_PENDING(true, 4, 8);
        nf_chunk<NT, 1, false>(acc, st.wb, bj, st.bias);
    }
    nf_net_store_raw<NT>(acc, sigma_raw, p0, n_points, lane, raw);
}

static int nf_lcode_launch_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                               const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream) {
    constexpr int NT = NF_MLP_NT;
    static_assert(NF_MLP_WAVES * 16 * NT == 128, "nf_mlp_fwd_launch sizes the grid for 128 points per workgroup");
    const float* rdv = rd_view ? rd_view : rd;
    return nf_mlp_fwd_launch(saved ? NF_FWD_TRAIN_F32 : NF_FWD_INFER, packed, cond, ro, rd, z, raw, saved, n_rays, n_samples,
                             [&](int64_t n_points, unsigned grid) {
        if (saved)
            hipLaunchKernelGGL((k_lcode_mlp_fwd_save<NT>), dim3(grid), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream), packed, cond, ro, rd, rdv, z,
                               n_points, n_samples, raw, saved);
        else
            hipLaunchKernelGGL((k_lcode_mlp_fwd<NT>), dim3(grid), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream), packed, cond, ro, rd, rdv, z,
                               n_points, n_samples, raw);
    });
}

extern "C" int nf_lcode_mlp_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream) {
    return nf_lcode_launch_fwd(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, nullptr, stream);
}

// + one point tile of mask words (the exact-f32 masks are kept per 16-point tile)
// (sized for the split training layout too: its sections are n_points rounded up to 32 points long, nf_mlp_bf16_machinery.inc)
extern "C" size_t nf_lcode_saved_floats(int64_t n_points) { return (size_t)nlc::SAVED_PER_POINT * (size_t)((n_points + 31) & ~(int64_t)31) + 5 * 128; }

// Training forward: also fills `saved` (nf_lcode_saved_floats(n_points) floats), which nf_lcode_mlp_bwd reads.
extern "C" int nf_lcode_mlp_fwd_train(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                      const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream) {
    if (!saved) return NF_EINVAL;
    return nf_lcode_launch_fwd(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, saved, stream);
}
