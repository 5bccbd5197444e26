// K4 backward: gradients of the fused paper MLP w.r.t. all of its parameters and the latent code
// (reference: autograd through nerf/models.py:236-261; what is learnable is listed in SURVEY §8 A12).
//
// Three stages, all on exact-f32 MFMA (v_mfma_f32_16x16x4_f32):
//   B1  k_paper_mlp_bwd_chain   per 32-point wave tile, the forward kernel run in reverse on a transposed
//                               fragment image: dZ_l = (dZ_{l+1} . W_{l+1}) * [X_l > 0]; masks come from the
//                               activations the training forward saved; every dZ_l is written to HBM.
//   B2  k_dw_gemm (nf_mlp_dw.h)  dW_l = dZ_l^T . X_{l-1} as wave-level 128x128 output tiles with the point
//                               dimension (hundreds of thousands) split into slices; bias grads (column sums
//                               of dZ) fall out of the A fragments.  Deterministic: partial slabs per slice.
//   B3  k_grad_reduce /         sum the slabs over slices, then scatter into the 26 reference-layout tensors:
//       k_paper_grad_unpack     PE slot order -> reference columns, folded conditioning columns as outer
//                               products (db (x) [expr/3 | latent]), d latent = W[:,139:171]^T db.
// The three stages are written once for this family and the smaller paper model in nf_mlp_paper_net_bwd.h (NfPaperNet); this unit holds
// the family's kernels, record and entry points, and the backward driver every family's record goes through (nf_bwd_run).
#include <cstdlib>
#include "nf_mlp_paper_net_bwd.h"

static NfPackTable g_paper_table_t;

extern "C" size_t nf_paper_packed_bwd_floats(void) { return (size_t)NfPaperNet::PACKED_T; }

extern "C" int nf_paper_pack_bwd(const float* const* params, float* packed_t, nf_stream_t stream) {
    return nf_pack_f32<NfPaperNet::NPARAMS, 1>(g_paper_table_t, nf_paper_net_table_t<NfPaperNet>, params, packed_t, (int)NfPaperNet::PACKED_T, stream);
}

// B1 (nf_paper_net_bwd_chain)
template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_paper_mlp_bwd_chain_masks(const float* __restrict__ packed_t, const float* __restrict__ saved, const float* __restrict__ d_raw,
                             int64_t n_points, float* __restrict__ dz) {
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    nf_paper_net_bwd_chain<NfPaperNet, NT>(lds, packed_t, saved, d_raw, n_points, dz);
}

// B3, second half (nf_paper_net_grad_unpack)
__global__ void __launch_bounds__(256) k_paper_grad_unpack(const float* __restrict__ sum, const float* __restrict__ packed,
                                                           const float* __restrict__ cond, NfNetGradOffsets<NfPaperNet> offs,
                                                           float* __restrict__ grads) {
    nf_paper_net_grad_unpack<NfPaperNet>(sum, packed, cond, offs, grads);
}

extern "C" size_t nf_paper_grad_floats(void) { return (size_t)nfl::GRAD_FLOATS; }

// defined in nf_mlp_bf16_dw.hip
void nfb_dw_plan(int model, int64_t n_points, int64_t* pts_per_slice, int* n_slices);
int nfb_launch_dw_gemm_bf16(int model, const float* dz, const float* d_raw, const float* saved, int64_t n_points, int64_t pts_per_slice,
                            int n_slices, float* slabs, const float* gscale, nf_stream_t stream);
int nfb_launch_dw_gemm_f16(int model, const float* dz, const float* d_raw, const float* saved, int64_t n_points, int64_t pts_per_slice,
                           int n_slices, float* slabs, const float* gscale, nf_stream_t stream);

// =================================================================================================
// the backward driver of both families (nf_mlp_bwd.h)
// =================================================================================================
size_t nf_bwd_workspace_floats(const NfBwdFamily& fam, int64_t n_points) {
    int64_t pps; int ns, ns_b;
    nfb_dw_plan(fam.model, n_points, &pps, &ns);
    NfDwGroup groups[NF_DW_MAX_GROUPS];
    fam.build_groups(groups);
    ns_b = nf_dw_plan_groups(groups, fam.n_groups, n_points);
    if (ns_b > ns) ns = ns_b;
    return (size_t)fam.dz_per_point * (size_t)n_points + (size_t)(ns + 1) * fam.slab_floats + 16;      // + max |gradient| per dz section (fp16 kernels)
}

int nf_bwd_run(const NfBwdFamily& fam, int precision, const float* packed, const void* packed_t, const float* cond, const float* saved,
               const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads,
               nf_stream_t stream, float* stage_ms, const float* saved_f32) {
    if (!packed || !packed_t || !cond || !saved || !d_raw || !workspace || !grads || n_rays <= 0 || n_samples <= 0 || precision < 0 ||
        precision > 2)
        return NF_EINVAL;
    const bool split_dw = precision != 0 && !saved_f32;
    const int64_t n_points = n_rays * n_samples;
    const size_t need = nf_bwd_workspace_floats(fam, n_points);
    if (workspace_floats < need) return NF_EINVAL;
    // as the training forward: 32-bit byte offsets into a (32-padded) section; also bounds every grid below
    if (((n_points + 31) & ~(int64_t)31) >= ((int64_t)1 << 22)) return NF_EINVAL;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev < 0 || dev >= 64) return NF_EINVAL;
    int64_t pps = 0; int ns;
    NfDwGroupSet gset;
    NfReduceAlt alt;
    alt.n_slices = 0;
    for (int q = 0; q < NF_REDUCE_ALT_MAX; ++q) alt.lo4[q] = alt.hi4[q] = 0;
    // the slabs are fully written by the GEMM kernel -- except, in the shared-panel plan, by the group that runs fewer slices: the
    // reduction is told which regions end early instead of a 71 MB zero-fill per call
    bool zero_fill = true;
    if (split_dw) nfb_dw_plan(fam.model, n_points, &pps, &ns);
    else {
        fam.build_groups(gset.g);
        for (int k = 0; k <= NF_DW_MAX_GROUPS; ++k) gset.first_block[k] = 0x7fffffff;
        ns = nf_dw_plan_groups(gset.g, fam.n_groups, n_points, gset.first_block);
        zero_fill = !nf_dw_reduce_alt(gset.g, fam.n_groups, ns, &alt);
        if (zero_fill) alt.n_slices = 0;
    }
    float* dz = workspace;
    float* slabs = workspace + (size_t)fam.dz_per_point * n_points;
    float* sum = slabs + (size_t)ns * fam.slab_floats;
    float* gscale = workspace + need - 16;
    hipStream_t s = nf_s(stream);
    if (zero_fill) {
        e = hipMemsetAsync(slabs, 0, (size_t)ns * fam.slab_floats * sizeof(float), s);
        if (e != hipSuccess) return (int)e;
    }
    if (precision == 2) {
        e = hipMemsetAsync(gscale, 0, 16 * sizeof(float), s);           // max |gradient| per section, filled by the chain
        if (e != hipSuccess) return (int)e;
    }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};          // stage_ms: dX chain | weight-gradient GEMMs | reduce + unpack
    auto mark = [&](int k) {
        if (stage_ms && hipEventCreate(&ev[k]) == hipSuccess) (void)hipEventRecord(ev[k], s);
    };
    mark(0);
    int rc = fam.chain[precision](packed_t, saved, d_raw, n_points, dz, precision == 2 ? gscale : nullptr, stream);
    if (rc) return rc;
    mark(1);
    if (split_dw) {
        rc = precision == 2 ? nfb_launch_dw_gemm_f16(fam.model, dz, d_raw, saved, n_points, pps, ns, slabs, gscale, stream)
                            : nfb_launch_dw_gemm_bf16(fam.model, dz, d_raw, saved, n_points, pps, ns, slabs, nullptr, stream);
        if (rc) return rc;
    } else {
        fam.dw_f32(gset, dz, d_raw, saved_f32 ? saved_f32 : saved, n_points, slabs, s);
    }
    mark(2);
    fam.reduce_unpack(slabs, ns, alt, sum, packed, cond, grads, s);
    if (stage_ms) {
        mark(3);
        e = hipStreamSynchronize(s);
        for (int k = 0; k < 3; ++k) {
            stage_ms[k] = -1.0f;
            if (e == hipSuccess && ev[k] && ev[k + 1]) (void)hipEventElapsedTime(&stage_ms[k], ev[k], ev[k + 1]);
        }
        for (auto& x : ev)
            if (x) (void)hipEventDestroy(x);
        if (e != hipSuccess) return (int)e;
    }
    NF_RETURN_LAUNCH();
}

// =================================================================================================
// the paper model's record and entry points
// =================================================================================================
// defined in nf_mlp_bf16_bwd.hip / nf_mlp_f16_bwd.hip
int nfb_launch_bwd_chain_bf16(const void* packed_t, const float* saved, const float* d_raw, int64_t n_points, float* dz,
                              float* gscale, nf_stream_t stream);
int nfb_launch_bwd_chain_f16(const void* packed_t, const float* saved, const float* d_raw, int64_t n_points, float* dz,
                             float* gscale, nf_stream_t stream);

static int nf_paper_chain_f32(const void* packed_t, const float* saved, const float* d_raw, int64_t n_points, float* dz, float*,
                              nf_stream_t stream) {
    return nf_paper_net_chain_launch(k_paper_mlp_bwd_chain_masks<NF_MLP_NT>, packed_t, saved, d_raw, n_points, dz, stream);
}

static void nf_paper_reduce_unpack(const float* slabs, int ns, const NfReduceAlt& alt, float* sum, const float* packed, const float* cond,
                                   float* grads, hipStream_t s) {
    nf_paper_net_reduce_unpack<NfPaperNet>(k_paper_grad_unpack, slabs, ns, alt, sum, packed, cond, grads, s);
}

static const NfBwdFamily nf_paper_bwd = {NfPaperNet::MODEL, NfPaperNet::DZ_PER_POINT, NfPaperNet::SLAB_FLOATS, nf_net_dw_groups<NfPaperNet>,
                                         nf_paper_net_build_dw_groups<NfPaperNet>,
                                         {nf_paper_chain_f32, nfb_launch_bwd_chain_bf16, nfb_launch_bwd_chain_f16},
                                         nf_paper_net_dw_f32<NfPaperNet>, nf_paper_reduce_unpack};

extern "C" size_t nf_paper_bwd_workspace_floats(int64_t n_points) { return nf_bwd_workspace_floats(nf_paper_bwd, n_points); }

// Measurement hook (bench.py's per-kernel training roofline): one backward in arithmetic `precision` (0 exact f32, 1 split-bf16,
// 2 split-fp16; packed_t_any = the matching transposed image / stream) with HIP events recorded on `stream` between its stages;
// synchronises the stream and returns stage_ms[3] = {dX chain, weight-gradient GEMMs, slab reduction + unpack} in milliseconds.
extern "C" int nf_paper_mlp_bwd_stage_ms(const float* packed, const void* packed_t_any, int precision, const float* cond, const float* saved,
                                         const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                         float* grads, float* stage_ms, nf_stream_t stream) {
    if (!packed_t_any || !stage_ms || precision < 0 || precision > 2) return NF_EINVAL;
    return nf_bwd_run(nf_paper_bwd, precision, packed, packed_t_any, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats,
                      grads, stream, stage_ms);
}

extern "C" int nf_paper_mlp_bwd(const float* packed, const float* packed_t, const float* cond, const float* saved,
                                const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                float* grads, nf_stream_t stream) {
    return nf_bwd_run(nf_paper_bwd, 0, packed, packed_t, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads, stream);
}

// Same, with the dX chain (nf_mlp_bf16_bwd.hip) and, unless exact_dw, the weight-gradient GEMMs (nf_mlp_bf16_dw.hip) on the
// split-bf16 kernels.  `saved` must come from nf_paper_mlp_fwd_train_bf16 (it carries the ReLU bit masks the chain reads).
// saved_f32 (exact_dw only, else NULL): `saved` converted by nf_split_saved_to_f32 -- the exact-f32 GEMMs read f32 rows.
extern "C" int nf_paper_mlp_bwd_bf16(const float* packed, const void* packed_t_bf16, const float* cond, const float* saved,
                                     const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                     float* grads, int exact_dw, const float* saved_f32, nf_stream_t stream) {
    if (exact_dw && !saved_f32) return NF_EINVAL;
    return nf_bwd_run(nf_paper_bwd, 1, packed, packed_t_bf16, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads,
                      stream, nullptr, exact_dw ? saved_f32 : nullptr);
}

// Same on fp16 operand pairs ("f16x3": fp32-class accuracy at the split-bf16 speed): dX chain (nf_mlp_f16_bwd.hip) and weight-
// gradient GEMMs (nf_mlp_f16_dw.hip), gradients in block floating point (a power-of-two scale per point and layer in the chain, per dZ section in the GEMMs).  `saved` must
// come from nf_paper_mlp_fwd_train_f16; packed_t_f16 from nf_paper_pack_bwd_f16.
extern "C" int nf_paper_mlp_bwd_f16(const float* packed, const void* packed_t_f16, const float* cond, const float* saved,
                                    const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                    float* grads, nf_stream_t stream) {
    return nf_bwd_run(nf_paper_bwd, 2, packed, packed_t_f16, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads,
                      stream);
}

// host-only self-test of the exact-f32 group table (tests/test_host.py)
extern "C" int nf_selftest_dw_tables_f32(void) { return nf_paper_net_selftest_dw_tables<NfPaperNet>(); }
