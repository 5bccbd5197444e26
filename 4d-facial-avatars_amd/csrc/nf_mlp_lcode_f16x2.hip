// "f16x2" forward of the second model family (ConditionalBlendshapeLearnableCodeNeRFModel, M:529-636): the kernel body of
// nf_mlp_lcode_bf16_kernel.inc on fp16 operands with two products per weight (W_hi.x_hi + W_lo.x_hi) -- see nf_mlp_f16x2.hip.
// Inference only; reads the packed image of nf_lcode_pack_f16.
#include <vector>
#include <mutex>

#define NFB_F16 1
#define NFB_PRODUCTS 5
#define NFB_TILE_GROUP 4
#define NFB_ACT_SHIFT 4
#include "nf_mlp_lcode_bf16_common.h"
#include "nf_pack.h"

#define NFB_SAVE 0
#define NFB_KERNEL_NAME k_lcode_mlp_fwd_f16x2
#include "nf_mlp_lcode_bf16_kernel.inc"

extern "C" int nf_lcode_mlp_fwd_f16x2(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                      const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream) {
    return nf_split_fwd(k_lcode_mlp_fwd_f16x2, NF_FWD_INFER, packed_f16, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, nullptr, stream);
}
