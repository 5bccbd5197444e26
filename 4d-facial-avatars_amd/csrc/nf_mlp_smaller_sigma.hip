// Density-only inference forward of ConditionalBlendshapePaperSmallerNeRFModel, exact f32: k_smaller_mlp_fwd (nf_mlp_smaller.hip) up
// to and including fc_alpha, one float per point (nf_paper_net_body<..., SIGMA>, nf_mlp_paper_net.h).  A translation unit of its own:
// see the header comment of nf_mlp_bf16_kernel.inc.
#include "nf_mlp_paper_net.h"

template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_smaller_mlp_sigma(const float* __restrict__ packed, const float* __restrict__ cond, const float* __restrict__ ro,
                    const float* __restrict__ rd, const float* __restrict__ z, int64_t n_points, int S, float* __restrict__ sigma) {
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    nf_paper_net_fwd_sigma<NfSmallerNet, NT>(lds, packed, cond, ro, rd, z, n_points, S, sigma);
}

extern "C" int nf_smaller_mlp_sigma(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                    const float* z, int64_t n_rays, int n_samples, float* sigma, nf_stream_t stream) {
    (void)rd_view;                                         // the direction never reaches fc_alpha
    return nf_paper_net_launch_sigma(k_smaller_mlp_sigma<NF_MLP_NT>, packed, cond, ro, rd, z, n_rays, n_samples, sigma, stream);
}
