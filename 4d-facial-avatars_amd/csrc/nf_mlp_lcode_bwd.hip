// Backward of the second model family (ConditionalBlendshapeLearnableCodeNeRFModel, reference nerf/models.py:529-636;
// autograd through M:590-636 as the trainer drives it, TR:355-392): gradients w.r.t. its 16 parameter tensors and the
// latent code, exact f32, same three stages as the paper model (nf_mlp_bwd.hip):
//   B1 k_lcode_mlp_bwd_chain   dZ_dir -> dZ_feat -> dZ_x2 (+ d sigma * fc_alpha.weight: fc_alpha reads x) -> dZ_x1 -> dZ_x0
//                              -> dZ_layer1 (layer1 has no activation), masks from the saved post-ReLU activations
//   B2 k_dw_gemm<1>            dW = dZ^T . X over point slices (24 wave jobs), bias grads as column sums
//   B3 k_grad_reduce<1>, k_lcode_grad_unpack   slabs -> the 16 reference-layout tensors (PE slot order -> columns, folded
//                              expression / latent / (near, far) columns as outer products) + d latent = W1[:,139:171]^T db1
#include <vector>
#include <mutex>
#include "nf_mlp_lcode_net_bwd.h"

// =================================================================================================
// transposed pack: block (ni, no), lane (g, i), r -> W[row = 16 ni + 4 g + r][col = 16 no + i]
// =================================================================================================
void nf_lcode_build_table_t(std::vector<uint32_t>& t, const NfLcodeGeom& ge) {
    using namespace nlc;
    const int* id = ge.id;
    t.assign(PACKED_T, NF_ZERO_CODE);
    auto fill = [&](int off, int nk, int no_tiles, int tensor, int n_rows, int n_cols) { nf_fill_frag_t(t, off, nk, no_tiles, tensor, n_rows, n_cols); };
    fill(OFFT_RGB, 1, 8, id[12], 3, 128);                       // fc_rgb.weight (3, 128)
    fill(OFFT_DIR, 8, 16, id[8], 128, 280);                     // layers_dir.0.weight[:, :256]
    fill(OFFT_FEAT, 16, 16, id[14], 256, 256);                  // fc_feat.weight
    fill(OFFT_FEAT + 16 * 16 * FRAG, 1, 16, id[10], 1, 256);    // chunk 16, slot 0: fc_alpha.weight (1, 256)
    fill(OFFT_X2, 16, 16, id[6], 256, 256);
    fill(OFFT_X1, 16, 16, id[4], 256, 256);
    fill(OFFT_X0, 16, 16, id[2], 256, 256);
}

static void nf_lcode_table_t(std::vector<uint32_t>& t) { nf_lcode_build_table_t(t, NF_LCODE_GEOM); }

static NfPackTable g_lcode_table_t;

extern "C" size_t nf_lcode_packed_bwd_floats(void) { return (size_t)nlc::PACKED_T; }

extern "C" int nf_lcode_pack_bwd(const float* const* params, float* packed_t, nf_stream_t stream) {
    return nf_pack_f32<nlc::NPARAMS, 5>(g_lcode_table_t, nf_lcode_table_t, params, packed_t, (int)nlc::PACKED_T, stream);
}

// =================================================================================================
// B1: backward chain
// =================================================================================================
// The layer list on the shared chain text (nf_mlp_net_common.h: NF_NET_CHAIN_*), like the paper model's (nf_mlp_paper_net_bwd.h).
// ReLU layers: layers_xyz.0..2 -> 0..2, fc_feat -> 3, layers_dir.0 -> 4.
template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_lcode_mlp_bwd_chain(const float* __restrict__ packed_t, const float* __restrict__ saved, const float* __restrict__ d_raw,
                      int64_t n_points, float* __restrict__ dz) {
    using namespace nlc;
    using Net = NfLcodeNet;
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    // d(layers_dir.0 out) = d rgb . fc_rgb.weight, masked by its ReLU
    NF_NET_CHAIN_BEGIN(4, OFFT_DIR / 4, 16);
    // d feat = dZ_dir . layers_dir.0.weight[:, :256], masked by relu(fc_feat)
    NF_NET_CHAIN_LAYER(OFFT_DIR / 4, 16, 8, 32, Z_DIR, 3, OFFT_FEAT / 4, 16);
    // d x2 = dZ_feat . fc_feat.weight + d sigma * fc_alpha.weight, masked by layers_xyz.2's ReLU: 16 slab chunks + one register chunk
    {
        f32x4 wd[16];
        nf_load_w16<16>(wd, Wi, OFFT_FEAT / 4 + 16 * 16 * 64, lane);
        NfCopyH<64, 4, false> cs{act4, sec(Z_FEAT, 256), lane, 8, {}};
        cs.prime();
        masks(2, m);
        nf_seg_lds<NT, 16, true, false, false>(acc, st, Wi, OFFT_FEAT / 4, 16, act4, lane, cs, unused64);
        nf_pending_b<NT, false>(bj, st);
        nf_chunk<NT, 16, false>(acc, st.wb, bj, st.bias);
        nf_tail_dz<NT, 16, 16, true>(acc, wd, frag_sig, st, Wi, OFFT_X2 / 4, act4, lane, m);
    }
    NF_NET_CHAIN_LAYER(OFFT_X2 / 4, 16, 16, 64, Z_X2, 1, OFFT_X1 / 4, 16);
    NF_NET_CHAIN_LAYER(OFFT_X1 / 4, 16, 16, 64, Z_X1, 0, OFFT_X0 / 4, 16);
    NF_NET_CHAIN_LAYER(OFFT_X0 / 4, 16, 16, 64, Z_X0, -1, 0, 0);              // d(layer1 out): layer1 has no activation (M:609)
    NF_NET_CHAIN_END(Z_L1);
}

// =================================================================================================
// B2 job table
// =================================================================================================
// the 24 products (128 x 128 each) as groups of four that share operand panels (k_dw_gemm_lds, nf_mlp_dw.h)
#define NF_LC_DW_GROUPS 6
static void nf_lcode_build_dw_groups(NfDwGroup* gr) {
    using namespace nlc;
    int n = 0;
    const NfDwPanel off{-1, 0, 0, 0, 0};
    auto fresh = [&]() -> NfDwGroup& {
        NfDwGroup& g = gr[n++];
        for (auto& p : g.panel) p = off;
        g.share = 2;
        g.n_slices = g.pts_per_slice = 0;
        return g;
    };
    auto job = [](const NfDwGroup& g, int a, int b, int out_off, int ldo, int cs) {
        return NfDwWaveJob{a, b, g.panel[a].valid, g.panel[b].valid, out_off, ldo, cs};
    };
    auto layer256 = [&](int zsec, int bsec, int gout, int cs) {
        NfDwGroup& g = fresh();
        for (int h = 0; h < 2; ++h) {
            g.panel[h] = NfDwPanel{0, zsec, 256, 128 * h, 128};
            g.panel[2 + h] = NfDwPanel{2, bsec, 256, 128 * h, 128};
        }
        for (int nb = 0; nb < 2; ++nb)
            for (int kb = 0; kb < 2; ++kb)
                g.wave[2 * nb + kb] = job(g, nb, 2 + kb, gout + 128 * nb * 256 + 128 * kb, 256, kb == 0 ? cs + 128 * nb : -1);
    };
    layer256(Z_X0, S_L1, G_X0, CS_L1 + 256);
    layer256(Z_X1, S_X0, G_X1, CS_L1 + 512);
    layer256(Z_X2, S_X1, G_X2, CS_L1 + 768);
    layer256(Z_FEAT, S_X2, G_FEAT, CS_L1 + 1024);
    {   // dZ_L1 x PE (two row blocks), dZ_dir x (dir slots | feat columns 0..127)
        NfDwGroup& g = fresh();
        g.panel[0] = NfDwPanel{0, Z_L1, 256, 0, 128};
        g.panel[1] = NfDwPanel{0, Z_L1, 256, 128, 128};
        g.panel[2] = NfDwPanel{2, S_PE, 64, 0, 64};
        g.panel[3] = NfDwPanel{0, Z_DIR, 128, 0, 128};
        g.panel[4] = NfDwPanel{2, S_DIRF, 16, 0, 16};
        g.panel[5] = NfDwPanel{2, S_FEAT, 256, 0, 128};
        g.wave[0] = job(g, 0, 2, G_L1, 64, CS_L1);
        g.wave[1] = job(g, 1, 2, G_L1 + 128 * 64, 64, CS_L1 + 128);
        g.wave[2] = job(g, 3, 4, G_DIRB, 16, -1);
        g.wave[3] = job(g, 3, 5, G_DIRA, 256, CS_DIR);
    }
    {   // dZ_dir x feat columns 128..255; d_raw x (dir-layer output | x2): rows 0..2 = fc_rgb.weight, row 3 (d sigma) = fc_alpha.weight
        NfDwGroup& g = fresh();
        g.panel[0] = NfDwPanel{0, Z_DIR, 128, 0, 128};
        g.panel[1] = NfDwPanel{2, S_FEAT, 256, 128, 128};
        g.panel[2] = NfDwPanel{1, 0, 4, 0, 4};
        g.panel[3] = NfDwPanel{2, S_DIR, 128, 0, 128};
        g.panel[4] = NfDwPanel{2, S_X2, 256, 0, 128};
        g.panel[5] = NfDwPanel{2, S_X2, 256, 128, 128};
        g.wave[0] = job(g, 0, 1, G_DIRA + 128, 256, -1);
        g.wave[1] = job(g, 2, 3, G_RGB, 128, CS_RGB);
        g.wave[2] = job(g, 2, 4, G_ALPHA, 256, -1);
        g.wave[3] = job(g, 2, 5, G_ALPHA + 128, 256, -1);
    }
    // n == NF_LC_DW_GROUPS by construction
}

// =================================================================================================
// B3, second half: scatter to the reference parameter layout (order = nerf.models.LCODE_KEYS)
// =================================================================================================
// the last workgroup: d latent_j = sum_n layer1.weight[n][139 + j] * d b1[n]
__global__ void __launch_bounds__(256) k_lcode_grad_unpack(const float* __restrict__ sum, const float* __restrict__ packed,
                                                           const float* __restrict__ cond, NfLcodeGradOffsets<171> offs,
                                                           float* __restrict__ grads) {
    using namespace nlc;
    if (blockIdx.x == gridDim.x - 1) {
        nf_lcode_dcond(packed, sum, 76, 32, grads + GRAD_PARAM_FLOATS);
        return;
    }
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < GRAD_PARAM_FLOATS; e += (gridDim.x - 1) * blockDim.x)
        grads[e] = nf_lcode_trunk_grad<171>(e, offs, sum, cond + B_CVEC, cond + B_DVEC);
}

extern "C" size_t nf_lcode_grad_floats(void) { return (size_t)nlc::GRAD_FLOATS; }

// defined in nf_mlp_lcode_bf16_bwd.hip / nf_mlp_lcode_f16_bwd.hip
int nfb_lcode_launch_bwd_chain_bf16(const void* packed_t, const float* saved, const float* d_raw, int64_t n_points, float* dz,
                                    float* gscale, nf_stream_t stream);
int nfb_lcode_launch_bwd_chain_f16(const void* packed_t, const float* saved, const float* d_raw, int64_t n_points, float* dz,
                                   float* gscale, nf_stream_t stream);

static int nf_lcode_chain_f32(const void* packed_t, const float* saved, const float* d_raw, int64_t n_points, float* dz, float*,
                              nf_stream_t stream) {
    const int64_t per_block = (int64_t)NF_MLP_WAVES * 16 * NF_MLP_NT;
    hipLaunchKernelGGL((k_lcode_mlp_bwd_chain<NF_MLP_NT>), dim3((unsigned)((n_points + per_block - 1) / per_block)), dim3(64 * NF_MLP_WAVES),
                       0, nf_s(stream), (const float*)packed_t, saved, d_raw, n_points, dz);
    return 0;
}

static void nf_lcode_dw_f32(const NfDwGroupSet& gset, const float* dz, const float* d_raw, const float* saved, int64_t n_points,
                            float* slabs, hipStream_t s) {
    hipLaunchKernelGGL((k_dw_gemm_lds<1>), dim3(gset.first_block[NF_LC_DW_GROUPS]), dim3(64 * NF_DW_WAVES), 0, s, gset, (int)nlc::SLAB_FLOATS,
                       dz, d_raw, saved, n_points, slabs);
}

// grads: nf_lcode_grad_floats() floats = the 16 tensors in nerf.models.LCODE_KEYS order, flattened, then d latent (32)
static void nf_lcode_reduce_unpack(const float* slabs, int ns, const NfReduceAlt& alt, float* sum, const float* packed, const float* cond,
                                   float* grads, hipStream_t s) {
    hipLaunchKernelGGL((k_grad_reduce<1>), dim3(512), dim3(256), 0, s, slabs, ns, (int)nlc::SLAB_FLOATS, sum, alt);
    hipLaunchKernelGGL(k_lcode_grad_unpack, dim3(1024 + 1), dim3(256), 0, s, sum, packed, cond, nf_lcode_grad_offsets<171>(),
                       grads);                                                                                      // + 1: the d-latent workgroup
}

static const NfBwdFamily nf_lcode_bwd = {1, nlc::DZ_PER_POINT, nlc::SLAB_FLOATS, NF_LC_DW_GROUPS, nf_lcode_build_dw_groups,
                                         {nf_lcode_chain_f32, nfb_lcode_launch_bwd_chain_bf16, nfb_lcode_launch_bwd_chain_f16},
                                         nf_lcode_dw_f32, nf_lcode_reduce_unpack};

// the same record with another scatter kernel behind the slab reduction: the classes of nf_mlp_bshape.hip / nf_mlp_cbshape.hip
void nf_lcode_grad_reduce(const float* slabs, int ns, const NfReduceAlt& alt, float* sum, hipStream_t s) {
    hipLaunchKernelGGL((k_grad_reduce<1>), dim3(512), dim3(256), 0, s, slabs, ns, (int)nlc::SLAB_FLOATS, sum, alt);
}

NfBwdFamily nf_lcode_bwd_family(void (*reduce_unpack)(const float*, int, const NfReduceAlt&, float*, const float*, const float*, float*,
                                                      hipStream_t)) {
    NfBwdFamily fam = nf_lcode_bwd;
    fam.reduce_unpack = reduce_unpack;
    return fam;
}

extern "C" size_t nf_lcode_bwd_workspace_floats(int64_t n_points) { return nf_bwd_workspace_floats(nf_lcode_bwd, n_points); }

extern "C" int nf_lcode_mlp_bwd(const float* packed, const float* packed_t, const float* cond, const float* saved, const float* d_raw,
                                int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads,
                                nf_stream_t stream) {
    return nf_bwd_run(nf_lcode_bwd, 0, packed, packed_t, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads, stream);
}

// Same on the split-bf16 kernels (dX chain nf_mlp_lcode_bf16_bwd.hip, weight-gradient GEMMs nf_mlp_bf16_dw.hip); `saved` must come
// from nf_lcode_mlp_fwd_train_bf16 (it carries the ReLU bit masks the chain reads).
extern "C" int nf_lcode_mlp_bwd_bf16(const float* packed, const void* packed_t_bf16, const float* cond, const float* saved,
                                     const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                     float* grads, nf_stream_t stream) {
    return nf_bwd_run(nf_lcode_bwd, 1, packed, packed_t_bf16, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads,
                      stream);
}

// Same on fp16 operand pairs ("f16x3"): `saved` from nf_lcode_mlp_fwd_train_f16, packed_t_f16 from nf_lcode_pack_bwd_f16.
extern "C" int nf_lcode_mlp_bwd_f16(const float* packed, const void* packed_t_f16, const float* cond, const float* saved,
                                    const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                    float* grads, nf_stream_t stream) {
    return nf_bwd_run(nf_lcode_bwd, 2, packed, packed_t_f16, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads,
                      stream);
}

// Measurement hook (tools/time_blendshape.py), as nf_paper_mlp_bwd_stage_ms: one backward in arithmetic `precision` (0 exact f32, 1 split-bf16,
// 2 split-fp16; packed_t_any: the matching transposed image / stream) with HIP events between its stages; synchronises the stream.
extern "C" int nf_lcode_mlp_bwd_stage_ms(const float* packed, const void* packed_t_any, int precision, const float* cond, const float* saved,
                                         const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                         float* grads, float* stage_ms, nf_stream_t stream) {
    if (precision < 0 || precision > 2 || !stage_ms) return NF_EINVAL;
    return nf_bwd_run(nf_lcode_bwd, precision, packed, packed_t_any, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads,
                      stream, stage_ms);
}

// host-only self-test of this family's exact-f32 group table (tests/test_host.py)
extern "C" int nf_selftest_dw_tables_lcode_f32(void) {
    NfDwGroup groups[NF_LC_DW_GROUPS];
    nf_lcode_build_dw_groups(groups);
    const long lcode = 256L * 64 + 4L * 65536 + 128L * 272 + 4L * 128 + 4L * 256 + 5 * 256 + 128 + 4;
    int rc = nf_check_dw_groups(groups, NF_LC_DW_GROUPS, nlc::SLAB_FLOATS, lcode);
    if (rc) return rc;
    for (int64_t n : {(int64_t)131072, (int64_t)262144, (int64_t)259969, (int64_t)512}) {
        int first[NF_DW_MAX_GROUPS + 1];
        const int most = nf_dw_plan_groups(groups, NF_LC_DW_GROUPS, n, first);
        NfReduceAlt alt;
        if (first[NF_LC_DW_GROUPS] > 256 || most < 1 || !nf_dw_reduce_alt(groups, NF_LC_DW_GROUPS, most, &alt) || alt.n_slices != 0) return -200;
    }
    return 0;
}
