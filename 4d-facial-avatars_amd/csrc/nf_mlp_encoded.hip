// ConditionalBlendshapePaperNeRFModel.forward on PRE-ENCODED inputs (reference nerf/models.py:236-261 as called by
// run_network, nerf/train_utils.py:20-24): x (P, 87) = [PE10(xyz) (63) | PE4(dirs) (24)] -> (P, 4).  Inference only; the
// hot path (run_one_iter_of_nerf) never materialises x and uses nf_paper_mlp_fwd instead.  Own translation unit on purpose;
// the network itself is nf_paper_net_fwd_encoded (nf_mlp_paper_net.h).
#include "nf_mlp_paper_net.h"

// bias table without the direction fold: the 24 direction columns arrive with x
__global__ void __launch_bounds__(256) k_paper_condition_encoded(const float* __restrict__ packed, const float* __restrict__ expr,
                                                                 const float* __restrict__ latent, float* __restrict__ cond) {
    nf_paper_net_condition<NfPaperNet, false>(packed, expr, latent, 0.0f, 0.0f, cond);
}

template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_paper_mlp_fwd_encoded(const float* __restrict__ packed, const float* __restrict__ cond, const float* __restrict__ x87,
                        int64_t n_points, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    nf_paper_net_fwd_encoded<NfPaperNet, NT>(lds, packed, cond, x87, n_points, out);
}

// x87: (n_points, 87) pre-encoded inputs; cond: scratch of nf_paper_cond_floats() floats; out: (n_points, 4).
extern "C" int nf_paper_forward_encoded(const float* packed, const float* x87, const float* expr76, const float* latent32,
                                        int64_t n_points, float* cond, float* out, nf_stream_t stream) {
    return nf_paper_net_forward_encoded(
        packed, x87, expr76, latent32, n_points, cond, out,
        [&] { hipLaunchKernelGGL(k_paper_condition_encoded, nf_paper_net_condition_grid<NfPaperNet>(), dim3(256), 0, nf_s(stream), packed, expr76, latent32, cond); },
        [&](unsigned grid) { hipLaunchKernelGGL((k_paper_mlp_fwd_encoded<NF_MLP_NT>), dim3(grid), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream), packed, cond, x87, n_points, out); });
}
