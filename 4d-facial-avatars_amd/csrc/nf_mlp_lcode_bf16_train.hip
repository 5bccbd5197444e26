// Training (activation-saving) instantiation of the split-bf16 fused forward of the second model family; its own translation
// unit so that it cannot perturb the code generation of the inference kernel (nf_mlp_lcode_bf16.hip).
#define NFB_TILE_GROUP 4          // two accumulator sets (deferred saves): A fragments of 4 output tiles at a time, no spills (8: 11 spilled registers)
#include "nf_mlp_lcode_bf16_common.h"

#define NFB_SAVE 1
#define NFB_KERNEL_NAME k_lcode_mlp_fwd_bf16_train
#include "nf_mlp_lcode_bf16_kernel.inc"

// Training forward on the split-bf16 kernel: also fills `saved` (nf_lcode_saved_floats(n_points) floats: the f32 sections of the
// exact-f32 training forward plus the ReLU bit masks nf_lcode_mlp_bwd_bf16 reads).
extern "C" int nf_lcode_mlp_fwd_train_bf16(const void* packed_bf16, const float* cond, const float* ro, const float* rd,
                                           const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,
                                           float* saved, nf_stream_t stream) {
    return nf_split_fwd(k_lcode_mlp_fwd_bf16_train, NF_FWD_TRAIN_SPLIT, packed_bf16, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, saved,
                        stream);
}
