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
// folded into the bias table by nf_smaller_condition: 6788 MFMAs per 16 points against the paper kernel's 7812.  The network itself is
// written once for both families in nf_mlp_paper_net.h (NfSmallerNet); this unit holds the family's kernels and entry points.
#include "nf_mlp_paper_net.h"

// =================================================================================================
// pack: gather the 22 nn.Parameter storages into the fragment-ordered image (nf_paper_net_table)
// =================================================================================================
static NfPackTable g_smaller_table;

extern "C" size_t nf_smaller_packed_floats(void) { return (size_t)nsm::PACKED; }
// 2076 floats are written; rounded up to whole KiB
extern "C" size_t nf_smaller_cond_floats(void) { return (size_t)((nsm::COND_FLOATS + 255) & ~255); }

// Host-side copy of the gather table (for layout tests without a GPU): code = tensor_id << 24 | offset.
extern "C" int nf_smaller_gather_table(uint32_t* out, size_t n) {
    if (!out || n != (size_t)nsm::PACKED) return NF_EINVAL;
    return nf_export_table(nf_paper_net_table<NfSmallerNet>, out, n) == (long)n ? 0 : NF_EINVAL;
}

extern "C" int nf_smaller_pack(const float* const* params, float* packed, nf_stream_t stream) {
    return nf_pack_f32<nsm::NPARAMS, 8>(g_smaller_table, nf_paper_net_table<NfSmallerNet>, params, packed, (int)nsm::PACKED, stream);
}

// =================================================================================================
// condition: per-call bias table (nf_paper_net_condition).  DIRS = false: pre-encoded inputs, no direction fold.
// =================================================================================================
template <bool DIRS>
__global__ void __launch_bounds__(256) k_smaller_condition(const float* __restrict__ packed, const float* __restrict__ expr,
                                                           const float* __restrict__ latent, float near_z, float far_z,
                                                           float* __restrict__ cond) {
    nf_paper_net_condition<NfSmallerNet, DIRS>(packed, expr, latent, near_z, far_z, cond);
}

extern "C" int nf_smaller_condition(const float* packed, const float* expr76, const float* latent32, float near_z, float far_z,
                                    float* cond, nf_stream_t stream) {
    if (!packed || !expr76 || !latent32 || !cond) return NF_EINVAL;
    hipLaunchKernelGGL(k_smaller_condition<true>, nf_paper_net_condition_grid<NfSmallerNet>(), dim3(256), 0, nf_s(stream), packed, expr76,
                       latent32, near_z, far_z, cond);
    NF_RETURN_LAUNCH();
}

// =================================================================================================
// forward
// =================================================================================================
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
    nf_net_inputs<NT>(pe, dirf, p0, n_points, S, lane, ro, rd, rd_view, z);
    f32x4 acc[NT][16];
    float sigma_raw[NT];
    const NfW Wi = nf_w_image(W, PACKED), Ci = nf_w_image(cond, COND_FLOATS);
    nf_paper_net_body<NfSmallerNet, NT, 1>(acc, sigma_raw, pe, dirf, Wi, Ci, act4, lane);
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
// x (P, 87) = [PE10(xyz) (63) | PE4(dirs) (24)] -> (P, 4).  Inference only (nf_paper_net_fwd_encoded).
template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_smaller_mlp_fwd_encoded(const float* __restrict__ packed, const float* __restrict__ cond, const float* __restrict__ x87,
                          int64_t n_points, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    nf_paper_net_fwd_encoded<NfSmallerNet, NT>(lds, packed, cond, x87, n_points, out);
}

// x87: (n_points, 87) pre-encoded inputs; cond: scratch of nf_smaller_cond_floats() floats; out: (n_points, 4).
extern "C" int nf_smaller_forward_encoded(const float* packed, const float* x87, const float* expr76, const float* latent32,
                                          int64_t n_points, float* cond, float* out, nf_stream_t stream) {
    return nf_paper_net_forward_encoded(
        packed, x87, expr76, latent32, n_points, cond, out,
        [&] { hipLaunchKernelGGL(k_smaller_condition<false>, nf_paper_net_condition_grid<NfSmallerNet>(), dim3(256), 0, nf_s(stream), packed, expr76, latent32, 0.0f, 0.0f, cond); },
        [&](unsigned grid) { hipLaunchKernelGGL((k_smaller_mlp_fwd_encoded<NF_MLP_NT>), dim3(grid), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream), packed, cond, x87, n_points, out); });
}

// Training forward (exact f32): the same arithmetic as k_smaller_mlp_fwd, plus everything the backward needs in `saved` (layout
// nsm::S_*; nf_paper_net_body_save)
template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_smaller_mlp_fwd_save(const float* __restrict__ packed, const float* __restrict__ cond, const float* __restrict__ ro,
                       const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z,
                       int64_t n_points, int S, float* __restrict__ raw, float* __restrict__ saved) {
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    nf_paper_net_fwd_save<NfSmallerNet, NT>(lds, packed, cond, ro, rd, rd_view, z, n_points, S, raw, saved);
}

static int nf_smaller_launch_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                 const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream) {
    return nf_paper_net_launch_fwd(k_smaller_mlp_fwd<NF_MLP_NT>, k_smaller_mlp_fwd_save<NF_MLP_NT>, packed, cond, ro, rd, rd_view, z, n_rays,
                                   n_samples, raw, saved, stream);
}

extern "C" int nf_smaller_mlp_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                  const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream) {
    return nf_smaller_launch_fwd(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, nullptr, stream);
}

extern "C" size_t nf_smaller_saved_floats(int64_t n_points) { return nf_paper_net_saved_floats<NfSmallerNet>(n_points); }

// Training forward: also fills `saved` (nf_smaller_saved_floats(n_points) floats), which nf_smaller_mlp_bwd reads.
extern "C" int nf_smaller_mlp_fwd_train(const float* packed, const float* cond, const float* ro, const float* rd,
                                        const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,
                                        float* saved, nf_stream_t stream) {
    if (!saved) return NF_EINVAL;
    return nf_smaller_launch_fwd(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, saved, stream);
}
