// What every (hi, lo) weight stream of the split-precision kernels derives from its layer table, written once.  Included behind a
// namespace nfb { NL, KS[], NO[] } -- a family's forward table (nf_mlp_bf16_common.h, nf_mlp_lcode_bf16_common.h) or the table of its
// transposed backward stream (nf_mlp_bf16_bwd.hip, nf_mlp_lcode_bf16_bwd.hip); a translation unit sees exactly one such table.
#pragma once
#include "nf_pack.h"

namespace nfb {
constexpr int pair_off(int l) { int o = 0; for (int i = 0; i < l; ++i) o += KS[i] * NO[i]; return o; }
constexpr int N_PAIRS = pair_off(NL);                 // (hi, lo) 1-KiB block pairs
constexpr int STREAM_BF16 = N_PAIRS * 2 * 512;        // 16-bit elements

// the stream's layer boundaries (NL + 1 pair offsets): what the fp16 pack kernels find a block's layer scale by
static inline void fill_pair_off(int* off) {
    for (int l = 0; l <= NL; ++l) off[l] = pair_off(l);
}
static inline NfLayerPairs<NL> layer_pairs() {
    NfLayerPairs<NL> lp;
    fill_pair_off(lp.off);
    return lp;
}

// Gather table of the stream: layer l, k-step s, output tile nt is one block pair; its entry of lane (h, i), slot j is
// code(l, s, nt, h, i, j) (NF_ZERO_CODE: a zero).
template <class Code>
static void fill_table(std::vector<uint32_t>& t, Code code) {
    t.assign((size_t)N_PAIRS * 512, NF_ZERO_CODE);
    for (int l = 0; l < NL; ++l)
        for (int s = 0; s < KS[l]; ++s)
            for (int nt = 0; nt < NO[l]; ++nt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j)
                        t[((size_t)(pair_off(l) + s * NO[l] + nt)) * 512 + lane * 8 + j] = code(l, s, nt, lane >> 5, lane & 31, j);
}
}  // namespace nfb
