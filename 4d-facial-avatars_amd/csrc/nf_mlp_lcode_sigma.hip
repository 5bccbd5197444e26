// Density-only inference forward of the second model family, exact f32: k_lcode_mlp_fwd (nf_mlp_lcode.hip) up to and including
// fc_alpha, one float per point (nf_lcode_net_body<..., SIGMA>, nf_mlp_lcode_net.h).  The two blendshape classes wrap it as they wrap
// the full forward (nf_mlp_bshape.h).  A translation unit of its own: see the header comment of nf_mlp_bf16_kernel.inc.
#include "nf_mlp_lcode_net.h"

template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_lcode_mlp_sigma(const float* __restrict__ packed, const float* __restrict__ cond, const float* __restrict__ ro,
                  const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z, int64_t n_points, int S,
                  float* __restrict__ raw) {
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p0 = ((int64_t)blockIdx.x * NF_MLP_WAVES + wave) * (16 * NT);
    if (p0 >= n_points) return;
    f32x4* act4 = lds + wave * (16 * NT * 64);
    f32x4 pe[NT][4];
    f32x4 dirf[NT][1];
    nf_net_inputs<NT>(pe, dirf, p0, n_points, S, lane, ro, rd, rd_view, z);
    f32x4 acc[NT][16];
    float sigma_raw[NT];
    const NfW Wi = nf_w_image(packed, nlc::PACKED), Ci = nf_w_image(cond, nlc::COND_FLOATS);
    nf_lcode_net_body<NT, 1, true>(acc, sigma_raw, pe, dirf, Wi, Ci, act4, lane);
    if ((lane >> 4) == 0) {                                // `raw` is sigma[n_points]
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int64_t p = p0 + 16 * t + (lane & 15);
            if (p < n_points) raw[p] = sigma_raw[t];
        }
    }
}

extern "C" int nf_lcode_mlp_sigma(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                  const float* z, int64_t n_rays, int n_samples, float* sigma, nf_stream_t stream) {
    constexpr int NT = NF_MLP_NT;
    static_assert(NF_MLP_WAVES * 16 * NT == 128, "nf_mlp_fwd_launch sizes the grid for 128 points per workgroup");
    (void)rd_view;                                         // the direction never reaches fc_alpha
    return nf_mlp_fwd_launch(NF_FWD_INFER, packed, cond, ro, rd, z, sigma, nullptr, n_rays, n_samples, [&](int64_t n_points, unsigned grid) {
        hipLaunchKernelGGL((k_lcode_mlp_sigma<NT>), dim3(grid), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream), packed, cond, ro, rd, rd, z,
                           n_points, n_samples, sigma);
    });
}
