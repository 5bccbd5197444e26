// Training (activation-saving) instantiation of the split-bf16 fused forward; its own translation unit so that it cannot
// perturb the code generation of the inference kernel (nf_mlp_bf16.hip).
#include "nf_mlp_bf16_common.h"

#define NFB_SAVE 1
#define NFB_KERNEL_NAME k_paper_mlp_fwd_bf16_train
#include "nf_mlp_bf16_kernel.inc"

// Training forward on the split-bf16 kernel: also fills `saved` (nf_paper_saved_floats(n_points) floats, f32, the layout
// nf_paper_mlp_bwd reads) plus the ReLU bit masks nf_paper_mlp_bwd_bf16 reads (S_MASK).
extern "C" int nf_paper_mlp_fwd_train_bf16(const void* packed_bf16, const float* cond, const float* ro, const float* rd,
                                           const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,
                                           float* saved, nf_stream_t stream) {
    if (!saved) return NF_EINVAL;
    return nf_split_fwd(k_paper_mlp_fwd_bf16_train, NF_FWD_TRAIN_SPLIT, packed_bf16, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, saved,
                        stream);
}
