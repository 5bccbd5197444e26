// B1 of the second model family on the bf16 matrix pipe: the backward chain of nf_mlp_lcode_bwd.hip as split-bf16 (3 bf16
// MFMAs per product, f32 accumulate), the mirror image of nf_mlp_lcode_bf16_kernel.inc on a TRANSPOSED (hi, lo) weight stream.
// The chain itself is nf_mlp_split_bwd.inc; this file holds the family's layer table, transposed-table rule, pack entry points
// and layer list.  ReLU gates come from the bit masks the split-bf16 training forward wrote (nlc::S_MASK); every dZ is written
// to HBM in f32 for the weight-gradient GEMMs.
//   0 fc_rgb^T (3 -> 128)   1 layers_dir.0[:, :256]^T (128 -> 256)   2 [fc_feat ; fc_alpha]^T (256 + 1 -> 256)
//   3 layers_xyz.2^T   4 layers_xyz.1^T   5 layers_xyz.0^T (-> dZ of layer1, which has no activation)
#include <vector>
#include <mutex>
#include "nf_mlp_split_common.h"
#include "nf_mlp_lcode_layout.h"

// NFB_F16 = 1 (nf_mlp_lcode_f16_bwd.hip includes this file): the same chain on fp16 operand pairs with per-point gradient scales
#if NFB_F16
#define NFB_TILE_GROUP 4
#endif

namespace nfb {
constexpr int NL = 6;
constexpr int KS[NL] = {2, 8, 18, 16, 16, 16};
constexpr int NO[NL] = {4, 8, 8, 8, 8, 8};
}  // namespace nfb
#include "nf_mlp_split_table.h"
#include "nf_mlp_bf16_machinery.inc"

// =================================================================================================
// transposed (hi, lo) stream: block (s, nt), lane (h', i), j  ->  W[row = reduction feature(s, h', j)][col = 32 nt + i]
// =================================================================================================

void nf_lcode_build_table_bf16_t(std::vector<uint32_t>& t, const NfLcodeGeom& ge);
#if !NFB_F16       // one definition: this file is compiled a second time as nf_mlp_lcode_f16_bwd.hip
void nf_lcode_build_table_bf16_t(std::vector<uint32_t>& t, const NfLcodeGeom& ge) {
    using namespace nfb;
    const int* id = ge.id;
    fill_table(t, [&](int l, int s, int nt, int h, int i, int j) {
        const int col = 32 * nt + i, row = hid_feature(s, h, j);
        uint32_t c = NF_ZERO_CODE;
        switch (l) {
            case 0: if (s == 0 && h == 0 && j < 3) c = nf_code(id[12], j, col, 128); break;      // slots 0..2 carry d r, d g, d b
            case 1: if (row < 128) c = nf_code(id[8], row, col, 280); break;
            case 2:                                                                      // k-step 16, slot (0, 0): d sigma
                if (s < 16) c = nf_code(id[14], row, col, 256);
                else if (s == 16 && h == 0 && j == 0) c = nf_code(id[10], 0, col, 256);
                break;
            case 3: c = nf_code(id[6], row, col, 256); break;
            case 4: c = nf_code(id[4], row, col, 256); break;
            case 5: c = nf_code(id[2], row, col, 256); break;
        }
        return c;
    });
}
#else
// layer boundaries (NL + 1 pair offsets) of the transposed stream, for the classes that pack their own tensors into it
void nf_lcode_bwd_f16_stream_layers(int* pair_off) { nfb::fill_pair_off(pair_off); }
#endif

static void nf_lcode_table_bf16_t(std::vector<uint32_t>& t) { nf_lcode_build_table_bf16_t(t, NF_LCODE_GEOM); }

static NfPackTable g_lcode_table_bt;

#if NFB_F16
extern "C" size_t nf_lcode_packed_bwd_f16_bytes(void) { return (size_t)nfb::STREAM_BF16 * 2 + NF_F16_TAIL_BYTES; }

extern "C" int nf_lcode_pack_bwd_f16(const float* const* params, void* stream_out, nf_stream_t stream) {
    return nf_pack_split_f16<nlc::NPARAMS, 17, nfb::NL>(g_lcode_table_bt, nf_lcode_table_bf16_t, params, stream_out, nfb::N_PAIRS * 512,
                                                        nfb::layer_pairs(), 1.0f, stream);
}
#else
extern "C" size_t nf_lcode_packed_bwd_bf16_bytes(void) { return (size_t)nfb::STREAM_BF16 * 2; }

extern "C" int nf_lcode_pack_bwd_bf16(const float* const* params, void* stream_out, nf_stream_t stream) {
    return nf_pack_split_bf16<nlc::NPARAMS, 7>(g_lcode_table_bt, nf_lcode_table_bf16_t, params, stream_out, nfb::N_PAIRS * 512, stream);
}
#endif

// =================================================================================================
// B1 kernel: the second family's layer list around nf_mlp_split_bwd.inc
// =================================================================================================
struct NfbChain { static constexpr int S_MASK = nlc::S_MASK, N_MASKS = 5; };

__global__ void __launch_bounds__(256, 1)
NFB_BWD_NAME(k_lcode_mlp_bwd_chain)(const char* __restrict__ wstream, const float* __restrict__ saved, const float* __restrict__ d_raw,
                                    int64_t n_points, float* __restrict__ dz, float* __restrict__ gscale) {
    using namespace nlc;
#include "nf_mlp_split_bwd.inc"
    // mask indices: layers_xyz.0..2 -> 0..2, fc_feat -> 3, layers_dir.0 -> 4
    nfb_zero_tiles<4>(accA);
    NFB_LAYER(0, accA, th, tl);
    NFB_BWD_FINISH(0, accA, 4, 4, 0.0f);                               // dZ_DIR
    nfb_zero_tiles<8>(accB);
    NFB_BWD_RUN(1, accB, bh, bl, 4, accA, Z_DIR);
    NFB_BWD_FINISH(1, accB, 8, 3, fabsf(d.w));                         // dZ_FEAT
    // d x2 = dZ_feat . fc_feat.weight + d sigma * fc_alpha.weight (fc_alpha reads x), gated by layers_xyz.2's ReLU
#pragma unroll
    for (int s = 0; s < 16; ++s) { th[s] = bh[s]; tl[s] = bl[s]; }
    nfb_dsigma_kstep<16>(th, tl, h == 0 && live, d.w, G);
    nfb_zero_tiles<8>(accA);
    NFB_BWD_RUN(2, accA, th, tl, 8, accB, Z_FEAT);
    NFB_BWD_FINISH(2, accA, 8, 2, 0.0f);                               // dZ_X2
    nfb_zero_tiles<8>(accB);
    NFB_BWD_RUN(3, accB, bh, bl, 8, accA, Z_X2);
    NFB_BWD_FINISH(3, accB, 8, 1, 0.0f);                               // dZ_X1
    nfb_zero_tiles<8>(accA);
    NFB_BWD_RUN(4, accA, bh, bl, 8, accB, Z_X1);
    NFB_BWD_FINISH(4, accA, 8, 0, 0.0f);                               // dZ_X0
    nfb_zero_tiles<8>(accB);
    NFB_BWD_RUN(5, accB, bh, bl, 8, accA, Z_X0);
    NFB_BWD_LAST(5, accB, -1, Z_L1);                                   // layer1 has no activation: dZ_L1 = d(out)
}

int NFB_BWD_NAME(nfb_lcode_launch_bwd_chain)(const void* packed_t, const float* saved, const float* d_raw, int64_t n_points, float* dz,
                                             float* gscale, nf_stream_t stream) {
    return nf_split_bwd_chain(NFB_BWD_NAME(k_lcode_mlp_bwd_chain), packed_t, saved, d_raw, n_points, dz, gscale, stream);
}

#if !NFB_F16
// host-only: the gather table of this stream (one 32-bit code per bf16 element of the hi blocks: tensor id << 24 | element
// offset, 0xFF000000 = zero) for tests/test_host.py; out == NULL returns the number of entries.  Transposed stream of the second model family.
extern "C" long nf_lcode_stream_table_bwd_bf16(uint32_t* out, size_t n_entries) { return nf_export_table(nf_lcode_table_bf16_t, out, n_entries); }
#endif
