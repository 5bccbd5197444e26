// Layer table of the split-precision kernels of the paper model (forward stream), shared by the inference and the training
// translation units (nf_mlp_bf16.hip, nf_mlp_bf16_train.hip, nf_mlp_f16*.hip).
#pragma once
#include "nf_mlp_split_common.h"
#include "nf_mlp_layout.h"

namespace nfb {
// layer table of the bf16 stream: k-steps (16 slots each, always even) and 32-row output tiles
constexpr int NL = 11;
constexpr int KS[NL] = {4, 16, 16, 20, 16, 16, 16, 18, 8, 8, 8};   // multiples of the stage depth (2 k-steps); layers_dir.0: 16 feat + dir + ONE zero k-step (round 5: 3)
constexpr int NO[NL] = {8, 8, 8, 8, 8, 8, 8, 5, 4, 4, 1};
}  // namespace nfb
#include "nf_mlp_split_table.h"

// the sections of `saved` the shared forward text writes (nf_mlp_split_fwd.inc)
struct NfbSections { static constexpr int S_PE = nfl::S_PE, S_DIRF = nfl::S_DIRF, S_MASK = nfl::S_MASK; };
