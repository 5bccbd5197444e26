// K4: fused forward of ConditionalBlendshapePaperNeRFModel (reference nerf/models.py:189-261) together
// with run_network's input assembly (reference nerf/train_utils.py:9-33,78): pts = ro + rd*z, both
// positional encodings, the [xyz | expr | latent] / skip / [feat | dirs] concatenations and all 11
// live Linear layers -- one launch, nothing but (ro, rd, z) read and 16 B/point written.
//
// Structure (gfx950, exact-f32 MFMA v_mfma_f32_16x16x4_f32; see nf_mlp_layout.h for the fragment maths):
//   * one wavefront owns 16*NT consecutive points for the whole network; waves never communicate, so
//     the kernel has no barrier at all (block = 4 independent waves, one per SIMD, 512-VGPR budget);
//   * the layer output of a wave (NT x 16 tiles x 4 regs) is accumulated in registers, written once to
//     the wave's private LDS slab as 16-byte fragments (XOR-swizzled, conflict-free) and read back as
//     the next layer's B fragments -- one ds_read_b128 per 64 MFMAs;
//   * weights stream from L2 (2.2 MB image, shared by every workgroup) as perfectly coalesced 1-KiB
//     wave loads, one K-chunk ahead of the MFMAs that consume them (register double buffer);
//   * the 63-wide positional encoding lives in registers in B-fragment order (one sin / cos pair per two
//     slots) and is consumed twice (layers_xyz.0 and the skip input of layers_xyz.3);
//   * the per-call constant input columns (expression, latent code, PE(near), PE(far)) never enter
//     the GEMMs: nf_paper_condition folds them into bias vectors (the `cond` table).
#include "nf_mlp_paper_net.h"


// =================================================================================================
// pack: gather the 26 nn.Parameter storages into the fragment-ordered image (nf_paper_net_table)
// =================================================================================================
static NfPackTable g_paper_table;

extern "C" size_t nf_paper_packed_floats(void) { return (size_t)NfPaperNet::PACKED; }
// 2332 floats are written; the buffer is padded to 10 KiB so that the bf16 kernel can DMA it into LDS in whole KiB blocks
extern "C" size_t nf_paper_cond_floats(void) { return 2560; }

// Host-side copy of the gather table (for layout tests without a GPU): code = tensor_id << 24 | offset.
extern "C" int nf_paper_gather_table(uint32_t* out, size_t n) {
    if (!out || n != (size_t)NfPaperNet::PACKED) return NF_EINVAL;
    return nf_export_table(nf_paper_net_table<NfPaperNet>, out, n) == (long)n ? 0 : NF_EINVAL;
}

extern "C" int nf_paper_pack(const float* const* params, float* packed, nf_stream_t stream) {
    return nf_pack_f32<NfPaperNet::NPARAMS, 0>(g_paper_table, nf_paper_net_table<NfPaperNet>, params, packed, (int)NfPaperNet::PACKED, stream);
}

// =================================================================================================
// condition: per-call bias table (nf_paper_net_condition)
// =================================================================================================
__global__ void __launch_bounds__(256) k_paper_condition(const float* __restrict__ packed, const float* __restrict__ expr,
                                                         const float* __restrict__ latent, float near_z, float far_z,
                                                         float* __restrict__ cond) {
    nf_paper_net_condition<NfPaperNet, true>(packed, expr, latent, near_z, far_z, cond);
}

extern "C" int nf_paper_condition(const float* packed, const float* expr76, const float* latent32, float near_z, float far_z,
                                  float* cond, nf_stream_t stream) {
    if (!packed || !expr76 || !latent32 || !cond) return NF_EINVAL;
    hipLaunchKernelGGL(k_paper_condition, nf_paper_net_condition_grid<NfPaperNet>(), dim3(256), 0, nf_s(stream), packed, expr76,
                       latent32, near_z, far_z, cond);
    NF_RETURN_LAUNCH();
}

// =================================================================================================
// forward
// =================================================================================================
template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_paper_mlp_fwd(const float* __restrict__ packed, const float* __restrict__ cond_, const float* __restrict__ ro,
                const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z,
                int64_t n_points, int S, float* __restrict__ raw) {
    using namespace nfl;
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15;
    f32x4* act4 = lds + wave * (16 * NT * 64);
    typedef __attribute__((address_space(1))) f32x4 nf_gf32x4;
    nf_gf32x4* raw_v = (nf_gf32x4*)raw;               // the output pointer and the grid stride live in VGPRs (see the epilogue)
    asm volatile("" : "+v"(raw_v));
    int stride_v = (int)gridDim.x;
    asm volatile("" : "+v"(stride_v));
    // persistent form: one workgroup per CU walks the point blocks with the grid's stride (no workgroup dispatch between blocks)
#pragma unroll 1
    for (int64_t blk = blockIdx.x;; blk += __builtin_amdgcn_readfirstlane(stride_v)) {
    const int64_t p0 = (blk * NF_MLP_WAVES + wave) * (16 * NT);
    if (p0 >= n_points) break;                        // wave-uniform; no barriers anywhere below
    int opaque0 = 0;                                  // per-block opaque zero: the weight / bias loads must stay where the layers issue them
    asm volatile("" : "+s"(opaque0));
    const f32x4* W = reinterpret_cast<const f32x4*>(packed) + opaque0;
    const float* cond = cond_ + opaque0;

    f32x4 pe[NT][4];
    f32x4 dirf[NT][1];
    nf_net_inputs<NT>(pe, dirf, p0, n_points, S, lane, ro, rd, rd_view, z);
    f32x4 acc[NT][16];
    float sigma_raw[NT];
    const NfW Wi = nf_w_image(reinterpret_cast<const float*>(W), PACKED_FLOATS), Ci = nf_w_image(cond, COND_FLOATS);
    nf_paper_net_body<NfPaperNet, NT, 1>(acc, sigma_raw, pe, dirf, Wi, Ci, act4, lane);
    // (the store predicate, the output pointer and the grid stride are re-derived from opaque VGPR copies: as loop invariants of the
    // persistent block loop they were the last scalar values the allocator could not keep -- 106 SGPRs are in use -- and went through
    // v_writelane / v_readlane)
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

// Training forward (exact f32): the same arithmetic as k_paper_mlp_fwd, plus everything the backward needs in `saved` (layout
// nfl::S_*; nf_paper_net_body_save)
template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_paper_mlp_fwd_save(const float* __restrict__ packed, const float* __restrict__ cond, const float* __restrict__ ro,
                     const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z,
                     int64_t n_points, int S, float* __restrict__ raw, float* __restrict__ saved) {
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    nf_paper_net_fwd_save<NfPaperNet, NT>(lds, packed, cond, ro, rd, rd_view, z, n_points, S, raw, saved);
}

static int nf_launch_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                         const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream) {
    return nf_paper_net_launch_fwd(k_paper_mlp_fwd<NF_MLP_NT>, k_paper_mlp_fwd_save<NF_MLP_NT>, packed, cond, ro, rd, rd_view, z, n_rays,
                                   n_samples, raw, saved, stream);
}

extern "C" int nf_paper_mlp_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream) {
    return nf_launch_fwd(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, nullptr, stream);
}

extern "C" size_t nf_paper_saved_floats(int64_t n_points) { return nf_paper_net_saved_floats<NfPaperNet>(n_points); }

extern "C" int nf_paper_mlp_fwd_train(const float* packed, const float* cond, const float* ro, const float* rd,
                                      const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,
                                      float* saved, nf_stream_t stream) {
    if (!saved) return NF_EINVAL;
    return nf_launch_fwd(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, saved, stream);
}
