// Split-fp16 ("f16x3") forward of the second model family (ConditionalBlendshapeLearnableCodeNeRFModel, M:529-636): the
// kernel body of nf_mlp_lcode_bf16_kernel.inc on fp16 operand pairs with per-layer power-of-two weight scales -- fp32-class
// accuracy at the split-bf16 speed; see nf_mlp_f16.hip for the scheme, the valid range and the range guard.
#include <vector>
#include <mutex>

#define NFB_F16 1
#define NFB_TILE_GROUP 4
#define NFB_ACT_SHIFT 4
#include "nf_mlp_lcode_bf16_common.h"
#include "nf_pack.h"

void nf_lcode_table_bf16_shared(std::vector<uint32_t>& t);          // nf_mlp_lcode_bf16.hip: same K order, same blocks

static NfPackTable g_lcode_table_h;

extern "C" size_t nf_lcode_packed_f16_bytes(void) { return (size_t)nfb::STREAM_BF16 * 2 + NF_F16_TAIL_BYTES; }
extern "C" size_t nf_lcode_f16_flag_offset(void) { return (size_t)nfb::STREAM_BF16 * 2 + 4 * NF_F16_FLAG_WORD; }

extern "C" int nf_lcode_pack_f16(const float* const* params, void* stream_out, nf_stream_t stream) {
    return nf_pack_split_f16<nlc::NPARAMS, 11, nfb::NL>(g_lcode_table_h, nf_lcode_table_bf16_shared, params, stream_out, nfb::N_PAIRS * 512,
                                                        nfb::layer_pairs(), (float)(1 << NFB_ACT_SHIFT), stream);
}

// the stream's layer boundaries (NL + 1 pair offsets) and activation pre-scale, for the classes that pack their own tensors into it
float nf_lcode_f16_stream_layers(int* pair_off) {
    nfb::fill_pair_off(pair_off);
    return (float)(1 << NFB_ACT_SHIFT);
}

#define NFB_SAVE 0
#define NFB_KERNEL_NAME k_lcode_mlp_fwd_f16
#include "nf_mlp_lcode_bf16_kernel.inc"

extern "C" int nf_lcode_mlp_fwd_f16(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                    const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream) {
    return nf_split_fwd(k_lcode_mlp_fwd_f16, NF_FWD_INFER, packed_f16, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, nullptr, stream);
}
