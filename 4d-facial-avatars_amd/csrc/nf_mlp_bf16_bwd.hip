// B1 on the bf16 matrix pipe: the backward chain dZ_l = (dZ_{l+1} . W_{l+1}) * [X_l > 0] of the paper MLP as split-bf16
// (3 bf16 MFMAs per product, f32 accumulate), the mirror image of nf_mlp_bf16_kernel.inc: gradients w.r.t. activations stay
// in registers from layer to layer, the TRANSPOSED weight stream (hi, lo fragment blocks) is staged L2 -> LDS through the same
// 4-deep ring.  ReLU masks come as bit masks written by the split-bf16 training forward (one 16-byte load per layer, all
// issued before the ring starts, so that no ordinary load sits in the pipelined part); every dZ_l is written to HBM in f32 for
// the weight-gradient GEMMs (split-bf16: nf_mlp_bf16_dw.hip; exact f32: nf_mlp_dw.h).
// The chain itself is nf_mlp_split_bwd.inc, shared with the second family (nf_mlp_lcode_bf16_bwd.hip); this file holds the paper
// model's layer table, transposed-table rule, pack entry points and layer list.
#include <vector>
#include <mutex>
#include "nf_mlp_split_common.h"
#include "nf_mlp_layout.h"

// NFB_F16 = 1 (nf_mlp_f16_bwd.hip includes this file): the same chain on fp16 operand pairs -- transposed weight stream with
// per-layer power-of-two scales (nf_pack.h), gradients carried times a per-POINT power of two chosen layer by layer from the
// point's largest gradient (block floating point, nf_mlp_bf16_machinery.inc) so that they sit at the top of fp16's exponent range.
#if NFB_F16
#define NFB_TILE_GROUP 4
#endif

namespace nfb {
// backward layers in execution order: reduction k-steps (over the forward layer's OUTPUT features) and 32-row output tiles
//   0 fc_rgb^T (3 -> 128)   1 layers_dir.2^T   2 layers_dir.1^T   3 [layers_dir.0[:, :256] ; fc_alpha]^T (128 + 1 -> 256)
//   4 fc_feat^T   5 layers_xyz.5^T   6 .4^T   7 .3[:, 171:]^T   8 .2^T   9 .1^T
constexpr int NL = 10;
constexpr int KS[NL] = {2, 8, 8, 10, 16, 16, 16, 16, 16, 16};
constexpr int NO[NL] = {4, 4, 4, 8, 8, 8, 8, 8, 8, 8};
}  // namespace nfb
#include "nf_mlp_split_table.h"
#include "nf_mlp_bf16_machinery.inc"

// =================================================================================================
// transposed (hi, lo) stream: block (s, nt), lane (h', i), j  ->  W[row = reduction feature(s, h', j)][col0 + 32 nt + i]
// =================================================================================================

static void nf_build_table_bf16_t(std::vector<uint32_t>& t) {
    using namespace nfb;
    // per layer: (tensor, rows valid, ncols, col0)
    const int tensor[NL] = {24, 20, 18, 16, 12, 10, 8, 6, 4, 2};
    const int nrows[NL] = {3, 128, 128, 128, 256, 256, 256, 256, 256, 256};
    const int ncols[NL] = {128, 128, 128, 280, 256, 256, 256, 427, 256, 256};
    const int col0[NL] = {0, 0, 0, 0, 0, 0, 0, 171, 0, 0};
    fill_table(t, [&](int l, int s, int nt, int h, int i, int j) {
        const int col = col0[l] + 32 * nt + i;
        uint32_t c = NF_ZERO_CODE;
        if (l == 0) {                                   // slots (s = 0, h = 0, j = 0..2) carry d r, d g, d b
            if (s == 0 && h == 0 && j < 3) c = nf_code(24, j, col, 128);
        } else if (l == 3) {                            // k-steps 0..7: dZ of layers_dir.0; k-step 8, slot (0, 0): d sigma
            if (s < 8) c = nf_code(16, hid_feature(s, h, j), col, 280);
            else if (s == 8 && h == 0 && j == 0) c = nf_code(14, 0, col, 256);
        } else {
            const int row = hid_feature(s, h, j);
            if (row < nrows[l]) c = nf_code(tensor[l], row, col, ncols[l]);
        }
        return c;
    });
}

static NfPackTable g_paper_table_bt;

#if NFB_F16
extern "C" size_t nf_paper_packed_bwd_f16_bytes(void) { return (size_t)nfb::STREAM_BF16 * 2 + NF_F16_TAIL_BYTES; }

extern "C" int nf_paper_pack_bwd_f16(const float* const* params, void* stream_out, nf_stream_t stream) {
    return nf_pack_split_f16<NF_PAPER_NUM_PARAMS, 13, nfb::NL>(g_paper_table_bt, nf_build_table_bf16_t, params, stream_out,
                                                               nfb::N_PAIRS * 512, nfb::layer_pairs(), 1.0f, stream);
}
#else
extern "C" size_t nf_paper_packed_bwd_bf16_bytes(void) { return (size_t)nfb::STREAM_BF16 * 2; }

extern "C" int nf_paper_pack_bwd_bf16(const float* const* params, void* stream_out, nf_stream_t stream) {
    return nf_pack_split_bf16<NF_PAPER_NUM_PARAMS, 3>(g_paper_table_bt, nf_build_table_bf16_t, params, stream_out, nfb::N_PAIRS * 512, stream);
}
#endif

// =================================================================================================
// B1 kernel: the paper model's layer list around nf_mlp_split_bwd.inc
// =================================================================================================
struct NfbChain { static constexpr int S_MASK = nfl::S_MASK, N_MASKS = 9; };

__global__ void __launch_bounds__(256, 1)
NFB_BWD_NAME(k_paper_mlp_bwd_chain)(const char* __restrict__ wstream, const float* __restrict__ saved, const float* __restrict__ d_raw,
                                    int64_t n_points, float* __restrict__ dz, float* __restrict__ gscale) {
    using namespace nfl;
#include "nf_mlp_split_bwd.inc"
    // mask indices: h0..h5 -> 0..5, layers_dir.0..2 outputs -> 6..8
    nfb_zero_tiles<4>(accA);
    NFB_LAYER(0, accA, th, tl);
    NFB_BWD_FINISH(0, accA, 4, 8, 0.0f);                               // dZ_D2
    nfb_zero_tiles<4>(accB);
    NFB_BWD_RUN(1, accB, bh, bl, 4, accA, Z_D2);
    NFB_BWD_FINISH(1, accB, 4, 7, 0.0f);                               // dZ_D1
    nfb_zero_tiles<4>(accA);
    NFB_BWD_RUN(2, accA, bh, bl, 4, accB, Z_D1);
    NFB_BWD_FINISH(2, accA, 4, 6, fabsf(d.w));                         // dZ_D0
    // d feat = dZ_D0 . layers_dir.0[:, :256] + d sigma * fc_alpha.weight (no activation on feat)
#pragma unroll
    for (int s = 0; s < 8; ++s) { th[s] = bh[s]; tl[s] = bl[s]; }
    nfb_dsigma_kstep<8>(th, tl, h == 0 && live, d.w, G);
    nfb_zero_tiles<8>(accB);
    NFB_BWD_RUN(3, accB, th, tl, 4, accA, Z_D0);
    NFB_BWD_FINISH(3, accB, 8, -1, 0.0f);                              // dZ_FEAT
    nfb_zero_tiles<8>(accA);
    NFB_BWD_RUN(4, accA, bh, bl, 8, accB, Z_FEAT);
    NFB_BWD_FINISH(4, accA, 8, 5, 0.0f);                               // dZ_L5
    nfb_zero_tiles<8>(accB);
    NFB_BWD_RUN(5, accB, bh, bl, 8, accA, Z_L5);
    NFB_BWD_FINISH(5, accB, 8, 4, 0.0f);                               // dZ_L4
    nfb_zero_tiles<8>(accA);
    NFB_BWD_RUN(6, accA, bh, bl, 8, accB, Z_L4);
    NFB_BWD_FINISH(6, accA, 8, 3, 0.0f);                               // dZ_L3
    nfb_zero_tiles<8>(accB);
    NFB_BWD_RUN(7, accB, bh, bl, 8, accA, Z_L3);
    NFB_BWD_FINISH(7, accB, 8, 2, 0.0f);                               // dZ_L2
    nfb_zero_tiles<8>(accA);
    NFB_BWD_RUN(8, accA, bh, bl, 8, accB, Z_L2);
    NFB_BWD_FINISH(8, accA, 8, 1, 0.0f);                               // dZ_L1
    nfb_zero_tiles<8>(accB);
    NFB_BWD_RUN(9, accB, bh, bl, 8, accA, Z_L1);
    NFB_BWD_LAST(9, accB, 0, Z_L0);                                    // dZ_L0
}

int NFB_BWD_NAME(nfb_launch_bwd_chain)(const void* packed_t, const float* saved, const float* d_raw, int64_t n_points, float* dz,
                                       float* gscale, nf_stream_t stream) {
    return nf_split_bwd_chain(NFB_BWD_NAME(k_paper_mlp_bwd_chain), packed_t, saved, d_raw, n_points, dz, gscale, stream);
}

#if !NFB_F16
// host-only: the gather table of this stream (one 32-bit code per bf16 element of the hi blocks: tensor id << 24 | element
// offset, 0xFF000000 = zero) for tests/test_host.py; out == NULL returns the number of entries.  Transposed (backward-chain) stream of the paper model.
extern "C" long nf_paper_stream_table_bwd_bf16(uint32_t* out, size_t n_entries) { return nf_export_table(nf_build_table_bf16_t, out, n_entries); }
#endif
