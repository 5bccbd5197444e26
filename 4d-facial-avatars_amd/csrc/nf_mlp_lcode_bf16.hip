// Second model family (ConditionalBlendshapeLearnableCodeNeRFModel, reference nerf/models.py:529-636), inference forward on
// the bf16 matrix pipe at fp32-class accuracy: the split-bf16 scheme and the machinery of nf_mlp_bf16.hip (3 bf16 MFMAs per
// product, K order chosen so that a layer's D registers are the next layer's B operands, weight stream L2 -> LDS through a
// 4-deep LDS-DMA ring) instantiated for this family's layer table:
//   0 layer1 (PE 4 k-steps -> 256, no activation)   1..3 layers_xyz.0..2 (ReLU)   4 fc_alpha (reads x: 256 -> 1)
//   5 fc_feat (ReLU)   6 layers_dir.0 ([feat | dir k-step | pad] -> 128, ReLU)   7 fc_rgb (128 -> 3)
// Same per-call bias table (`cond`, nf_lcode_condition) and packed-weight source tensors as the exact-f32 kernel
// (nf_mlp_lcode.hip).  Training instantiation: nf_mlp_lcode_bf16_train.hip; backward chain: nf_mlp_lcode_bf16_bwd.hip.
#include <vector>
#include <mutex>
#include "nf_mlp_lcode_bf16_common.h"
#include "nf_pack.h"

// =================================================================================================
// pack: fp32 parameters (nerf.models.LCODE_KEYS order) -> (hi, lo) bf16 fragment stream
// =================================================================================================

void nf_lcode_build_table_bf16(std::vector<uint32_t>& t, const NfLcodeGeom& ge) {
    using namespace nfb;
    const int* id = ge.id;
    fill_table(t, [&](int l, int s, int nt, int h, int i, int j) {
        const int n = 32 * nt + i;
        uint32_t c = NF_ZERO_CODE;
        switch (l) {
            case 0: { const int col = pe_col(s, h, j); if (col >= 0) c = nf_code(id[0], n, col, ge.ld1); } break;
            case 1: c = nf_code(id[2], n, hid_feature(s, h, j), 256); break;
            case 2: c = nf_code(id[4], n, hid_feature(s, h, j), 256); break;
            case 3: c = nf_code(id[6], n, hid_feature(s, h, j), 256); break;
            case 4: if (n == 0) c = nf_code(id[10], 0, hid_feature(s, h, j), 256); break;
            case 5: c = nf_code(id[14], n, hid_feature(s, h, j), 256); break;
            case 6:
                if (s < 16) c = nf_code(id[8], n, hid_feature(s, h, j), 280);
                else if (s == 16) { const int col = dir_col(h, j); if (col >= 0) c = nf_code(id[8], n, col, 280); }
                break;
            case 7: if (n < 3) c = nf_code(id[12], n, hid_feature(s, h, j), 128); break;
        }
        return c;
    });
}

static void nf_lcode_table_bf16(std::vector<uint32_t>& t) { nf_lcode_build_table_bf16(t, NF_LCODE_GEOM); }

void nf_lcode_table_bf16_shared(std::vector<uint32_t>& t) { nf_lcode_table_bf16(t); }        // also the split-fp16 stream's table

static NfPackTable g_lcode_table_b;

extern "C" size_t nf_lcode_packed_bf16_bytes(void) { return (size_t)nfb::STREAM_BF16 * 2; }

extern "C" int nf_lcode_pack_bf16(const float* const* params, void* stream_out, nf_stream_t stream) {
    return nf_pack_split_bf16<nlc::NPARAMS, 6>(g_lcode_table_b, nf_lcode_table_bf16, params, stream_out, nfb::N_PAIRS * 512, stream);
}

#define NFB_SAVE 0
#define NFB_KERNEL_NAME k_lcode_mlp_fwd_bf16
#include "nf_mlp_lcode_bf16_kernel.inc"

// cond must be the padded table nf_lcode_condition fills (nf_lcode_cond_floats() floats >= 10 KiB)
extern "C" int nf_lcode_mlp_fwd_bf16(const void* packed_bf16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                     const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream) {
    return nf_split_fwd(k_lcode_mlp_fwd_bf16, NF_FWD_INFER, packed_bf16, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, nullptr, stream);
}

// host-only: the gather table of this stream (one 32-bit code per bf16 element of the hi blocks: tensor id << 24 | element
// offset, 0xFF000000 = zero) for tests/test_host.py; out == NULL returns the number of entries.  Forward stream of the second model family.
extern "C" long nf_lcode_stream_table_bf16(uint32_t* out, size_t n_entries) { return nf_export_table(nf_lcode_table_bf16, out, n_entries); }
