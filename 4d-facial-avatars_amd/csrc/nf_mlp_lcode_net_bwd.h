// Backward half of the second family's exact-f32 network (nf_mlp_lcode_net.h), written once for the three classes that run on it:
// the scatter of the trunk's 16 tensors from the reduced gradient slab into the reference layout and the gradient of the vector
// folded into layer1's bias.  The dX chain's layer list is k_lcode_mlp_bwd_chain (nf_mlp_lcode_bwd.hip) on the shared chain text
// (nf_mlp_net_common.h).
#pragma once
#include "nf_mlp_lcode_net.h"
#include "nf_mlp_bwd.h"

// ---- what the family's backward translation units provide to the classes that run on it ----------------------------------
void nf_lcode_build_table_t(std::vector<uint32_t>& t, const NfLcodeGeom& ge);         // transposed image (nf_mlp_lcode_bwd.hip)
void nf_lcode_build_table_bf16_t(std::vector<uint32_t>& t, const NfLcodeGeom& ge);    // transposed stream (nf_mlp_lcode_bf16_bwd.hip)
void nf_lcode_bwd_f16_stream_layers(int* pair_off);                                   // 6 + 1 offsets
void nf_lcode_grad_reduce(const float* slabs, int ns, const NfReduceAlt& alt, float* sum, hipStream_t s);
NfBwdFamily nf_lcode_bwd_family(void (*reduce_unpack)(const float*, int, const NfReduceAlt&, float*, const float*, const float*, float*,
                                                      hipStream_t));

// first flat element of each trunk tensor (the 16 tensors of nerf.ops.LCODE_KEYS order), layer1.weight LD1 columns wide
template <int LD1>
struct NfLcodeGradOffsets { int off[nlc::NPARAMS + 1]; };

template <int LD1>
static inline NfLcodeGradOffsets<LD1> nf_lcode_grad_offsets() {
    const int numel[nlc::NPARAMS] = {256 * LD1, 256, 65536, 256, 65536, 256, 65536, 256,    // layer1, layers_xyz.0..2
                                     128 * 280, 128, 256, 1, 384, 3, 65536, 256};           // layers_dir.0, fc_alpha, fc_rgb, fc_feat
    NfLcodeGradOffsets<LD1> o;
    o.off[0] = 0;
    for (int i = 0; i < nlc::NPARAMS; ++i) o.off[i + 1] = o.off[i] + numel[i];
    return o;
}

// One trunk element of the flat gradient vector from the reduced slab: PE slot order -> columns, the folded columns as outer
// products (column sum of the layer's dZ) x (the constant it multiplied); cvec = the folded vector (cond + B_CVEC), dvec = the
// (near, far) direction features (cond + B_DVEC).
template <int LD1>
__device__ __forceinline__ float nf_lcode_trunk_grad(int e, const NfLcodeGradOffsets<LD1>& offs, const float* __restrict__ sum,
                                                     const float* __restrict__ cvec, const float* __restrict__ dvec) {
    using namespace nlc;
    int t = 0;
    while (e >= offs.off[t + 1]) ++t;
    const int local = e - offs.off[t];
    switch (t) {
        case 0: {  // layer1.weight [256][LD1] = [pe 63 | folded vector]
            const int n = local / LD1, col = local - LD1 * n;
            return col < 63 ? sum[G_L1 + n * 64 + nfl::pe_col_to_slot(col)] : sum[CS_L1 + n] * cvec[col - 63];
        }
        case 1: return sum[CS_L1 + local];
        case 2: return sum[G_X0 + local];
        case 3: return sum[CS_L1 + 256 + local];
        case 4: return sum[G_X1 + local];
        case 5: return sum[CS_L1 + 512 + local];
        case 6: return sum[G_X2 + local];
        case 7: return sum[CS_L1 + 768 + local];
        case 8: {  // layers_dir.0.weight [128][280] = [feat 256 | PE4(rd_z, near, far) 24]
            const int n = local / 280, col = local - 280 * n;
            if (col < 256) return sum[G_DIRA + n * 256 + col];
            const int q = col - 256, f = q / 6, rem = q - 6 * f, sc = rem / 3, comp = rem - 3 * sc;
            return comp == 0 ? sum[G_DIRB + n * 16 + 4 * f + sc] : sum[CS_DIR + n] * dvec[4 * f + 2 * sc + (comp - 1)];
        }
        case 9: return sum[CS_DIR + local];
        case 10: return sum[G_ALPHA + 3 * 256 + local];      // fc_alpha.weight [1][256] = row 3 (d sigma) of d_raw^T x
        case 11: return sum[CS_RGB + 3];
        case 12: return sum[G_RGB + local];                  // fc_rgb.weight [3][128]
        case 13: return sum[CS_RGB + local];
        case 14: return sum[G_FEAT + local];
        default: return sum[CS_L1 + 1024 + local];
    }
}

// Gradient of `count` (<= 32) entries of the folded vector, the job of one whole workgroup of 256 threads (one thread per entry
// through 256 dependent trips was the longest path of the launch):
//   dst[k] = sum_n layer1.weight[n][63 + col0 + k] * d b1[n]
// thread (q, k) sums n = 32 q .. 32 q + 31, the eight partial sums of a k are added in a fixed order.  dst may be LDS: the caller
// places the barrier before reading it.
__device__ __forceinline__ void nf_lcode_dcond(const float* __restrict__ packed, const float* __restrict__ sum, int col0, int count,
                                               float* dst) {
    __shared__ float part[8][32];
    const int tid = threadIdx.x, k = tid & 31, q = tid >> 5;
    float v = 0.f;
    if (k < count) {
        const float* w1 = packed + nlc::OFF_WC1 + col0 + k;
#pragma unroll 8
        for (int n = 32 * q; n < 32 * q + 32; ++n) v += w1[n * 108] * sum[nlc::CS_L1 + n];
    }
    part[q][k] = v;
    __syncthreads();
    if (tid < count) {
        float r = part[0][tid];
#pragma unroll
        for (int j = 1; j < 8; ++j) r += part[j][tid];
        dst[tid] = r;
    }
}
