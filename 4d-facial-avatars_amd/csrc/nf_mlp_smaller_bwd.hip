// Backward of the third model family (ConditionalBlendshapePaperSmallerNeRFModel, reference nerf/models.py:266-338; autograd
// through M:313-338 as the trainer drives it): gradients w.r.t. its 22 parameter tensors and the latent code, exact f32, the three
// stages of the paper model (nf_mlp_bwd.hip) driven through one NfBwdFamily record (nf_mlp_bwd.h):
//   B1 k_smaller_mlp_bwd_chain  dZ_D2 -> dZ_D1 -> dZ_D0 -> d feat (+ d sigma * fc_alpha.weight) -> dZ_L4 -> dZ_L3 -> dZ_L2 -> dZ_L1
//                               -> dZ_L0, masks from the bit masks the training forward saved
//   B2 k_dw_gemm_lds<2>         dW = dZ^T . X over point slices (8 groups of four 128 x 128 products), bias grads as column sums
//   B3 k_grad_reduce<2>, k_smaller_grad_unpack   slabs -> the 22 reference-layout tensors: PE slot order -> columns; every folded
//                               column as (column sum of the layer's dZ) x (the constant it multiplied): expression and latent in
//                               layers_xyz.0 / .3, and in layers_dir.0 the 16 near / far columns AND the 76 expression columns;
//                               d latent = W0[:,139:171]^T db0 + W3[:,139:171]^T db3 (the latent code does not reach layers_dir.0)
// All three stages are written once for this family and the paper model in nf_mlp_paper_net_bwd.h (NfSmallerNet).
#include "nf_mlp_paper_net_bwd.h"

static NfPackTable g_smaller_table_t;

extern "C" size_t nf_smaller_packed_bwd_floats(void) { return (size_t)nsm::PACKED_T; }

extern "C" int nf_smaller_pack_bwd(const float* const* params, float* packed_t, nf_stream_t stream) {
    return nf_pack_f32<nsm::NPARAMS, 9>(g_smaller_table_t, nf_paper_net_table_t<NfSmallerNet>, params, packed_t, (int)nsm::PACKED_T, stream);
}

// B1 (nf_paper_net_bwd_chain).  ReLU layers: layers_xyz.0..4 -> 0..4, layers_dir.0..2 -> 5..7.
template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_smaller_mlp_bwd_chain(const float* __restrict__ packed_t, const float* __restrict__ saved, const float* __restrict__ d_raw,
                        int64_t n_points, float* __restrict__ dz) {
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    nf_paper_net_bwd_chain<NfSmallerNet, NT>(lds, packed_t, saved, d_raw, n_points, dz);
}

// B3, second half (nf_paper_net_grad_unpack)
__global__ void __launch_bounds__(256) k_smaller_grad_unpack(const float* __restrict__ sum, const float* __restrict__ packed,
                                                             const float* __restrict__ cond, NfNetGradOffsets<NfSmallerNet> offs,
                                                             float* __restrict__ grads) {
    nf_paper_net_grad_unpack<NfSmallerNet>(sum, packed, cond, offs, grads);
}

extern "C" size_t nf_smaller_grad_floats(void) { return (size_t)nsm::GRAD_FLOATS; }

static int nf_smaller_chain_f32(const void* packed_t, const float* saved, const float* d_raw, int64_t n_points, float* dz, float*,
                                nf_stream_t stream) {
    return nf_paper_net_chain_launch(k_smaller_mlp_bwd_chain<NF_MLP_NT>, packed_t, saved, d_raw, n_points, dz, stream);
}

// this family has no split arithmetic: the record's split slots answer NF_EINVAL
static int nf_smaller_chain_none(const void*, const float*, const float*, int64_t, float*, float*, nf_stream_t) { return NF_EINVAL; }

static void nf_smaller_reduce_unpack(const float* slabs, int ns, const NfReduceAlt& alt, float* sum, const float* packed, const float* cond,
                                     float* grads, hipStream_t s) {
    nf_paper_net_reduce_unpack<NfSmallerNet>(k_smaller_grad_unpack, slabs, ns, alt, sum, packed, cond, grads, s);
}

static const NfBwdFamily nf_smaller_bwd = {NfSmallerNet::MODEL, nsm::DZ_PER_POINT, nsm::SLAB_FLOATS, nf_net_dw_groups<NfSmallerNet>,
                                           nf_paper_net_build_dw_groups<NfSmallerNet>,
                                           {nf_smaller_chain_f32, nf_smaller_chain_none, nf_smaller_chain_none},
                                           nf_paper_net_dw_f32<NfSmallerNet>, nf_smaller_reduce_unpack};

extern "C" size_t nf_smaller_bwd_workspace_floats(int64_t n_points) { return nf_bwd_workspace_floats(nf_smaller_bwd, n_points); }

// grads: nf_smaller_grad_floats() floats = the 22 tensors in state_dict order, flattened, then d latent (32)
extern "C" int nf_smaller_mlp_bwd(const float* packed, const float* packed_t, const float* cond, const float* saved,
                                  const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                  float* grads, nf_stream_t stream) {
    return nf_bwd_run(nf_smaller_bwd, 0, packed, packed_t, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads, stream);
}

// Measurement hook (tools/time_smaller.py), as nf_paper_mlp_bwd_stage_ms for the exact-f32 backward: stage_ms[3] (host) =
// {dX chain, weight-gradient GEMMs, slab reduction + unpack} in milliseconds; synchronises the stream.
extern "C" int nf_smaller_mlp_bwd_stage_ms(const float* packed, const float* packed_t, const float* cond, const float* saved,
                                           const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                           float* grads, float* stage_ms, nf_stream_t stream) {
    if (!stage_ms) return NF_EINVAL;
    return nf_bwd_run(nf_smaller_bwd, 0, packed, packed_t, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads,
                      stream, stage_ms);
}

// host-only self-test of this family's exact-f32 group table (tests/test_smaller_host.py)
extern "C" int nf_selftest_dw_tables_smaller_f32(void) { return nf_paper_net_selftest_dw_tables<NfSmallerNet>(); }
