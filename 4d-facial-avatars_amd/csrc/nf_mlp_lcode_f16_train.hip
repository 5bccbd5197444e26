// Training (activation-saving) instantiation of the split-fp16 forward of the second model family (cf. nf_mlp_f16_train.hip).
#define NFB_F16 1
#define NFB_TILE_GROUP 2          // A fragments of 2 output tiles at a time: with the transposing side job of the saves, 4 spill 15 registers
#define NFB_ACT_SHIFT 4
#include "nf_mlp_lcode_bf16_common.h"
#include "nf_pack.h"

#define NFB_SAVE 1
#define NFB_KERNEL_NAME k_lcode_mlp_fwd_f16_train
#include "nf_mlp_lcode_bf16_kernel.inc"

extern "C" int nf_lcode_mlp_fwd_train_f16(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                          const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream) {
    return nf_split_fwd(k_lcode_mlp_fwd_f16_train, NF_FWD_TRAIN_SPLIT, packed_f16, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, saved,
                        stream);
}
