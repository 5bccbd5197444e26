// ConditionalCompressedBlendshapeNeRFModel (reference nerf/models.py:750-868; the `*_nolcode_fixed_bg_256_compressed` configs) as
// those configs instantiate it: per point the second family's network (nf_mlp_lcode.hip) with layer1 reading [PE(63) | e3 (20)],
// e3 = relu(L2(relu(L1(relu(L0(expr)))))) with layers_expr = Linear 76 -> 38 -> 20 -> 20 (M:832-834: the expression is NOT divided by
// 3, a ReLU follows each layer); no latent code.  The encoder is constant per call: the condition kernel evaluates it and folds
// layer1.weight[:, 63:83] . e3 into layer1's bias, the gradient scatter carries its backward.  Per-point work runs on the second
// family's kernels (nf_mlp_bshape.h).
#include "nf_mlp_bshape.h"

static const NfLcodeGeom NF_CBSHAPE_GEOM = {{6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21}, ncb::LD1, ncb::D3};

// the trunk image, then the six encoder tensors row-major (parameters 0..5)
static void nf_cbshape_table(std::vector<uint32_t>& t) {
    using namespace ncb;
    nf_lcode_build_table(t, NF_CBSHAPE_GEOM);
    t.resize(PACKED, NF_ZERO_CODE);
    const int off[N_ENC] = {E_W0, E_B0, E_W1, E_B1, E_W2, E_B2}, numel[N_ENC] = {D1 * D0, D1, D2 * D1, D2, D3 * D2, D3};
    for (int p = 0; p < N_ENC; ++p)
        for (int i = 0; i < numel[p]; ++i) t[OFF_ENC + off[p] + i] = nf_code(p, 0, i, numel[p]);
}

// one encoder layer in LDS: out[i] = relu(b[i] + sum_k W[i][k] in[k]), fmaf in index order starting from the bias
template <int N_OUT, int N_IN>
__device__ __forceinline__ void nf_cb_enc_layer(const float* __restrict__ w, const float* __restrict__ b, const float* in, float* out) {
    const int i = threadIdx.x;
    if (i < N_OUT) {
        float s = b[i];
        for (int k = 0; k < N_IN; ++k) s = fmaf(w[i * N_IN + k], in[k], s);
        out[i] = fmaxf(s, 0.0f);
    }
    __syncthreads();
}

// Every workgroup evaluates the encoder (a few thousand FMAs) and then fills its share of the bias table; workgroup 0 also leaves
// expr, e1, e2, e3 behind the table for the backward.  B_CVEC holds e3 padded with zeros.
template <bool ENCODED>
__global__ void __launch_bounds__(256) k_cbshape_condition(const float* __restrict__ packed, const float* __restrict__ expr, float near_z,
                                                           float far_z, float* __restrict__ cond) {
    using namespace ncb;
    __shared__ float x0[D0], e1[D1], e2[D2];
    __shared__ float cvec[108];
    __shared__ float dvec[16];
    const int tid = threadIdx.x;
    const float* enc = packed + OFF_ENC;
    if (tid < D0) x0[tid] = expr[tid];
    if (tid < 108) cvec[tid] = 0.0f;
    if (!ENCODED && tid >= 128 && tid < 144) dvec[tid - 128] = nf_lcode_dvec(tid - 128, near_z, far_z);
    __syncthreads();
    nf_cb_enc_layer<D1, D0>(enc + E_W0, enc + E_B0, x0, e1);
    nf_cb_enc_layer<D2, D1>(enc + E_W1, enc + E_B1, e1, e2);
    nf_cb_enc_layer<D3, D2>(enc + E_W2, enc + E_B2, e2, cvec);
    if (blockIdx.x == 0) {
        if (tid < D0) cond[C_EXPR + tid] = x0[tid];
        if (tid < D1) cond[C_E1 + tid] = e1[tid];
        if (tid < D2) cond[C_E2 + tid] = e2[tid];
        if (tid < D3) cond[C_E3 + tid] = cvec[tid];
    }
    nf_lcode_bias_table<D3, ENCODED>(packed, cvec, dvec, cond);
}

extern "C" int nf_cbshape_condition(const float* packed, const float* expr76, const float* latent32, float near_z, float far_z,
                                    float* cond, nf_stream_t stream) {
    (void)latent32;                                        // accepted for the family-uniform signature; the class has no latent code
    if (!packed || !expr76 || !cond) return NF_EINVAL;
    hipLaunchKernelGGL(k_cbshape_condition<false>, dim3((nlc::COND_FLOATS + 255) / 256), dim3(256), 0, nf_s(stream), packed, expr76, near_z,
                       far_z, cond);
    NF_RETURN_LAUNCH();
}

extern "C" int nf_cbshape_forward_encoded(const float* packed, const float* x87, const float* expr76, const float* latent32,
                                          int64_t n_points, float* cond, float* out, nf_stream_t stream) {
    (void)latent32;
    if (n_points == 0) return 0;
    if (!packed || !x87 || !expr76 || !cond || !out || n_points < 0) return NF_EINVAL;
    hipLaunchKernelGGL(k_cbshape_condition<true>, dim3((nlc::COND_FLOATS + 255) / 256), dim3(256), 0, nf_s(stream), packed, expr76, 0.0f,
                       0.0f, cond);
    return nf_lcode_launch_fwd_encoded(packed, cond, x87, n_points, out, stream);
}

// backward of one encoder layer, the workgroup's 256 threads: dz = d_out . [out > 0] (on the post-ReLU value, as torch.relu's backward),
// d W = dz (x) in, d b = dz, d_in = W^T dz summed over the layer's units in index order
template <int N_OUT, int N_IN, bool WANT_DIN>
__device__ __forceinline__ void nf_cb_enc_layer_bwd(const float* __restrict__ w, const float* out, const float* in, float* d_out /* -> dz */,
                                                    float* d_in, float* __restrict__ g_w, float* __restrict__ g_b) {
    const int tid = threadIdx.x;
    if (tid < N_OUT) {
        const float dz = out[tid] > 0.0f ? d_out[tid] : 0.0f;
        d_out[tid] = dz;
        g_b[tid] = dz;
    }
    __syncthreads();
    for (int e = tid; e < N_OUT * N_IN; e += blockDim.x) g_w[e] = d_out[e / N_IN] * in[e % N_IN];
    if (WANT_DIN) {
        if (tid < N_IN) {
            float s = 0.0f;
            for (int k = 0; k < N_OUT; ++k) s = fmaf(w[k * N_IN + tid], d_out[k], s);
            d_in[tid] = s;
        }
        __syncthreads();
    }
}

// The 16 trunk tensors with 83 columns (d layer1.weight[n][63 + k] = cs_L1[n] e3[k]: B_CVEC holds e3); the last workgroup does the
// encoder's backward -- fixed summation order, no atomics -- and writes the 32 zeros of d latent.
__global__ void __launch_bounds__(256) k_cbshape_grad_unpack(const float* __restrict__ sum, const float* __restrict__ packed,
                                                             const float* __restrict__ cond, NfLcodeGradOffsets<ncb::LD1> offs,
                                                             float* __restrict__ grads) {
    using namespace ncb;
    if (blockIdx.x == gridDim.x - 1) {
        __shared__ float x0[D0], e1[D1], e2[D2], e3[D3], d1[D1], d2[D2], d3[D3];
        const int tid = threadIdx.x;
        if (tid < D0) x0[tid] = cond[C_EXPR + tid];
        if (tid < D1) e1[tid] = cond[C_E1 + tid];
        if (tid < D2) e2[tid] = cond[C_E2 + tid];
        if (tid < D3) e3[tid] = cond[C_E3 + tid];
        nf_lcode_dcond(packed, sum, 0, D3, d3);               // d e3[k] = sum_n layer1.weight[n][63 + k] d b1[n]
        __syncthreads();
        const float* enc = packed + OFF_ENC;
        nf_cb_enc_layer_bwd<D3, D2, true>(enc + E_W2, e3, e2, d3, d2, grads + E_W2, grads + E_B2);
        nf_cb_enc_layer_bwd<D2, D1, true>(enc + E_W1, e2, e1, d2, d1, grads + E_W1, grads + E_B1);
        nf_cb_enc_layer_bwd<D1, D0, false>(enc + E_W0, e1, x0, d1, nullptr, grads + E_W0, grads + E_B0);
        if (tid < 32) grads[GRAD_PARAM_FLOATS + tid] = 0.0f;
        return;
    }
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < GRAD_PARAM_FLOATS - ENC_FLOATS; e += (gridDim.x - 1) * blockDim.x)
        grads[ENC_FLOATS + e] = nf_lcode_trunk_grad<LD1>(e, offs, sum, cond + nlc::B_CVEC, cond + nlc::B_DVEC);
}

extern "C" size_t nf_cbshape_grad_floats(void) { return (size_t)ncb::GRAD_PARAM_FLOATS + 32; }

// grads: the 22 tensors in state_dict order (nerf.ops.CBSHAPE.keys: layers_expr.0..2, then the trunk), flattened, then 32 zeros (d latent)
static void nf_cbshape_reduce_unpack(const float* slabs, int ns, const NfReduceAlt& alt, float* sum, const float* packed, const float* cond,
                                     float* grads, hipStream_t s) {
    nf_lcode_grad_reduce(slabs, ns, alt, sum, s);
    hipLaunchKernelGGL(k_cbshape_grad_unpack, dim3(1024 + 1), dim3(256), 0, s, sum, packed, cond, nf_lcode_grad_offsets<ncb::LD1>(), grads);
}

NF_BSHAPE_SHARED_ENTRY_POINTS(nf_cbshape, NF_CBSHAPE_GEOM, ncb::NPARAMS, 50, nf_cbshape_table, ncb::PACKED)
