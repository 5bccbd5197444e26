// Density-only inference forward of the second model family, "f16x2": the kernel of nf_mlp_lcode_f16x2.hip up to and including
// fc_alpha, one float per point.  Same weight stream (the image of nf_lcode_pack_f16), ring, scales and range guard;
// the ring ends with the last layer that runs (NFB_RUN_LAYERS, nf_mlp_bf16_machinery.inc).  A translation unit of its own: see the
// header comment of nf_mlp_bf16_kernel.inc.
#include <vector>
#include <mutex>

#define NFB_F16 1
#define NFB_PRODUCTS 5            // bit 0: W_lo x_hi, bit 2: W_hi x_hi
#define NFB_TILE_GROUP 4
#define NFB_ACT_SHIFT 4
#define NFB_RUN_LAYERS 5
#define NFB_SIGMA_ONLY 1
#include "nf_mlp_lcode_bf16_common.h"
#include "nf_pack.h"

#define NFB_SAVE 0
#define NFB_KERNEL_NAME k_lcode_mlp_sigma_f16x2
#include "nf_mlp_lcode_bf16_kernel.inc"

extern "C" int nf_lcode_mlp_sigma_f16x2(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                        const float* z, int64_t n_rays, int n_samples, float* sigma, nf_stream_t stream) {
    return nf_split_fwd(k_lcode_mlp_sigma_f16x2, NF_FWD_INFER, packed_f16, cond, ro, rd, rd_view, z, n_rays, n_samples, sigma, nullptr, stream);
}
