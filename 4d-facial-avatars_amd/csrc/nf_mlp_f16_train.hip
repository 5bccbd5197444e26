// Training (activation-saving) instantiation of the split-fp16 fused forward (see nf_mlp_f16.hip for the scheme); its own
// translation unit like nf_mlp_bf16_train.hip.  `saved` receives the TRUE layer outputs (scales removed) in the layout the
// weight-gradient kernels read, plus the ReLU bit masks the split backward chain reads.
#define NFB_F16 1
#define NFB_TILE_GROUP 2          // A fragments of 2 output tiles at a time: with the transposing side job of the saves, 4 spill 15 registers
#define NFB_ACT_SHIFT 4
#include "nf_mlp_bf16_common.h"
#include "nf_pack.h"

#define NFB_SAVE 1
#define NFB_KERNEL_NAME k_paper_mlp_fwd_f16_train
#include "nf_mlp_bf16_kernel.inc"

// Training forward on the split-fp16 kernel: also fills `saved` (TRUE layer outputs, the layout nf_paper_mlp_bwd* read) and the
// ReLU bit masks the split backward chain reads.
extern "C" int nf_paper_mlp_fwd_train_f16(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                          const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream) {
    return nf_split_fwd(k_paper_mlp_fwd_f16_train, NF_FWD_TRAIN_SPLIT, packed_f16, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, saved,
                        stream);
}
