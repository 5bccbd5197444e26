// ConditionalBlendshapeNeRFModel (reference nerf/models.py:872-976; the `ji_nolcode_fixed_bg_256` configs) as those configs
// instantiate it (num_layers 4, hidden 256, no skip, 10/4 encoding functions): per point the second family's network
// (nf_mlp_lcode.hip) with layer1 reading [PE(63) | expr/3 (76)] -- no latent code (M:935: it arrives in **kwargs and is ignored).
// Per-point work runs on the second family's kernels (nf_mlp_bshape.h); here: the class's tables, bias table and gradient scatter.
#include "nf_mlp_bshape.h"

static const NfLcodeGeom NF_BSHAPE_GEOM = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, nbs::LD1, nbs::N_EXPR};

static void nf_bshape_table(std::vector<uint32_t>& t) { nf_lcode_build_table(t, NF_BSHAPE_GEOM); }

// k_lcode_condition with a 76-entry vector: a second-family model whose latent columns are zero gets the same table bit for bit
template <bool ENCODED>
__global__ void __launch_bounds__(256) k_bshape_condition(const float* __restrict__ packed, const float* __restrict__ expr, float near_z,
                                                          float far_z, float* __restrict__ cond) {
    __shared__ float cvec[108];
    __shared__ float dvec[16];
    const int tid = threadIdx.x;
    if (tid < 108) cvec[tid] = tid < nbs::N_EXPR ? nf_div(nf_mul(expr[tid], 1.0f), 3.0f) : 0.0f;
    if (!ENCODED && tid >= 128 && tid < 144) dvec[tid - 128] = nf_lcode_dvec(tid - 128, near_z, far_z);
    __syncthreads();
    nf_lcode_bias_table<nbs::N_EXPR, ENCODED>(packed, cvec, dvec, cond);
}

extern "C" int nf_bshape_condition(const float* packed, const float* expr76, const float* latent32, float near_z, float far_z,
                                   float* cond, nf_stream_t stream) {
    (void)latent32;                                        // accepted for the family-uniform signature; the class has no latent code
    if (!packed || !expr76 || !cond) return NF_EINVAL;
    hipLaunchKernelGGL(k_bshape_condition<false>, dim3((nlc::COND_FLOATS + 255) / 256), dim3(256), 0, nf_s(stream), packed, expr76, near_z,
                       far_z, cond);
    NF_RETURN_LAUNCH();
}

extern "C" int nf_bshape_forward_encoded(const float* packed, const float* x87, const float* expr76, const float* latent32,
                                         int64_t n_points, float* cond, float* out, nf_stream_t stream) {
    (void)latent32;
    if (n_points == 0) return 0;
    if (!packed || !x87 || !expr76 || !cond || !out || n_points < 0) return NF_EINVAL;
    hipLaunchKernelGGL(k_bshape_condition<true>, dim3((nlc::COND_FLOATS + 255) / 256), dim3(256), 0, nf_s(stream), packed, expr76, 0.0f,
                       0.0f, cond);
    return nf_lcode_launch_fwd_encoded(packed, cond, x87, n_points, out, stream);
}

// k_lcode_grad_unpack with 139 columns; the last workgroup writes the 32 zeros of d latent
__global__ void __launch_bounds__(256) k_bshape_grad_unpack(const float* __restrict__ sum, const float* __restrict__ cond,
                                                            NfLcodeGradOffsets<nbs::LD1> offs, float* __restrict__ grads) {
    if (blockIdx.x == gridDim.x - 1) {
        if (threadIdx.x < 32) grads[nbs::GRAD_PARAM_FLOATS + threadIdx.x] = 0.0f;
        return;
    }
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nbs::GRAD_PARAM_FLOATS; e += (gridDim.x - 1) * blockDim.x)
        grads[e] = nf_lcode_trunk_grad<nbs::LD1>(e, offs, sum, cond + nlc::B_CVEC, cond + nlc::B_DVEC);
}

extern "C" size_t nf_bshape_grad_floats(void) { return (size_t)nbs::GRAD_PARAM_FLOATS + 32; }

// grads: the 16 tensors in state_dict order (nerf.ops.BSHAPE.keys), flattened, then 32 zeros (d latent)
static void nf_bshape_reduce_unpack(const float* slabs, int ns, const NfReduceAlt& alt, float* sum, const float* packed, const float* cond,
                                    float* grads, hipStream_t s) {
    (void)packed;
    nf_lcode_grad_reduce(slabs, ns, alt, sum, s);
    hipLaunchKernelGGL(k_bshape_grad_unpack, dim3(1024 + 1), dim3(256), 0, s, sum, cond, nf_lcode_grad_offsets<nbs::LD1>(), grads);
}

NF_BSHAPE_SHARED_ENTRY_POINTS(nf_bshape, NF_BSHAPE_GEOM, 16, 40, nf_bshape_table, nlc::PACKED)
