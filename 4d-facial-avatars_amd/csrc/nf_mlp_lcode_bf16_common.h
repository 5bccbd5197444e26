// Layer table of the split-precision kernels of the second model family (forward stream), shared by the inference and the
// training translation units (nf_mlp_lcode_bf16.hip, nf_mlp_lcode_bf16_train.hip, nf_mlp_lcode_f16*.hip).
#pragma once
#include "nf_mlp_split_common.h"
#include "nf_mlp_lcode_layout.h"

namespace nfb {
constexpr int NL = 8;
constexpr int KS[NL] = {4, 16, 16, 16, 16, 16, 18, 8};   // layers_dir.0: 16 feat k-steps + the dir k-step + ONE zero k-step (a stage is 2 k-steps; round 5: 3)
constexpr int NO[NL] = {8, 8, 8, 8, 1, 8, 4, 1};
}  // namespace nfb
#include "nf_mlp_split_table.h"

// the sections of `saved` the shared forward text writes (nf_mlp_split_fwd.inc)
struct NfbSections { static constexpr int S_PE = nlc::S_PE, S_DIRF = nlc::S_DIRF, S_MASK = nlc::S_MASK; };
