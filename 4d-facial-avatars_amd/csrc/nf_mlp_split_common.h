// Shared by the split-precision kernels of both model families (forward streams, backward chains, weight-gradient GEMMs): the
// element-type switch, the family-independent slot helpers and the forward and backward-chain launches.  A family's header adds
// its layer table (namespace nfb { NL, KS[], NO[] }) and includes nf_mlp_split_table.h, which derives the rest from it.
#pragma once
#include "nf_common.h"

// Element type of the split operands.  NFB_F16 = 0: bf16 pairs (x = hi + lo keeps 16 significand bits, f32's exponent range);
// NFB_F16 = 1: fp16 pairs (22 significand bits -- fp32-class accuracy at the same three MFMAs per product; the narrow fp16
// exponent range is handled by a per-layer power-of-two weight scale chosen at pack time, see nf_mlp_f16.hip).
#ifndef NFB_F16
#define NFB_F16 0
#endif
#if NFB_F16
typedef _Float16 nfb_elt;
typedef _Float16 bf16x8 __attribute__((ext_vector_type(8)));      // (the name is historical: 8 split-operand elements of type nfb_elt)
#define NFB_MFMA __builtin_amdgcn_mfma_f32_32x32x16_f16
#else
typedef __bf16 nfb_elt;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#define NFB_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16
#endif
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace nfb {
// slot (s, h, j) of a hidden input -> feature index (D register order of the producing layer)
__host__ __device__ constexpr int hid_feature(int s, int h, int j) { return 16 * s + 4 * h + (j & 3) + 8 * (j >> 2); }
// PE slots: 4 k-steps; lane half h, step s, j: pair p = 16 h + 4 s + (j >> 1); sc = j & 1.
// p < 30: (freq, comp) = (p / 3, p % 3); p = 30: raw x, raw y; p = 31: raw z, zero pad.
__host__ __device__ constexpr int pe_col(int s, int h, int j) {
    const int p = 16 * h + 4 * s + (j >> 1), sc = j & 1;
    if (p < 30) return 3 + 6 * (p / 3) + 3 * sc + (p % 3);
    if (p == 30) return sc;            // x, y
    return sc == 0 ? 2 : -1;           // z, pad
}
// dir slots (one k-step): half h, j < 4: freq = 2 h + (j >> 1), sc = j & 1 -> layers_dir.0 column 256 + 6 f + 3 sc
__host__ __device__ constexpr int dir_col(int h, int j) { return j < 4 ? 256 + 6 * (2 * h + (j >> 1)) + 3 * (j & 1) : -1; }
}  // namespace nfb

// A split forward kernel (a family's layer list in nf_mlp_bf16_kernel.inc / nf_mlp_lcode_bf16_kernel.inc around the text both share,
// nf_mlp_split_fwd.inc): 256 threads per 128 points; saved = NULL for the
// inference instantiations
typedef void (*NfSplitFwdKernel)(const char* wstream, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                 const float* z, int64_t n_points, int n_samples, float* raw, float* saved);

static inline int nf_split_fwd(NfSplitFwdKernel kernel, NfFwdMode mode, const void* wstream, const float* cond, const float* ro,
                               const float* rd, const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,
                               float* saved, nf_stream_t stream) {
    return nf_mlp_fwd_launch(mode, wstream, cond, ro, rd, z, raw, saved, n_rays, n_samples, [&](int64_t n_points, unsigned grid) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, nf_s(stream), reinterpret_cast<const char*>(wstream), cond, ro, rd,
                           rd_view ? rd_view : rd, z, n_points, n_samples, raw, saved);
    });
}

// A split backward-chain kernel (a family's layer list in nf_mlp_bf16_bwd.hip / nf_mlp_lcode_bf16_bwd.hip around nf_mlp_split_bwd.inc),
// same tiling; the unit is compiled once per arithmetic and NFB_BWD_NAME keeps the two sets of names apart.
// gscale: 16 zeroed words on the device that receive max |dz| per layer (fp16 instantiation; ignored by the bf16 one)
#if NFB_F16
#define NFB_BWD_NAME(x) x##_f16
#else
#define NFB_BWD_NAME(x) x##_bf16
#endif
typedef void (*NfSplitBwdChainKernel)(const char* wstream, const float* saved, const float* d_raw, int64_t n_points, float* dz, float* gscale);

static inline int nf_split_bwd_chain(NfSplitBwdChainKernel kernel, const void* packed_t, const float* saved, const float* d_raw,
                                     int64_t n_points, float* dz, float* gscale, nf_stream_t stream) {
    const int64_t grid = (n_points + 127) / 128;
    if (grid > 0x7fffffff) return NF_EINVAL;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, nf_s(stream), reinterpret_cast<const char*>(packed_t), saved, d_raw,
                       n_points, dz, gscale);
    NF_RETURN_LAUNCH();
}
