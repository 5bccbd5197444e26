// Host-side backward driver shared by the two fused MLP families (nf_mlp_bwd.hip: the paper model, nf_mlp_lcode_bwd.hip: the
// learnable-code model).  A family is described by an NfBwdFamily record; its kernels stay in its own translation unit and are
// reached through the launchers of the record.
#pragma once
#include "nf_mlp_dw.h"

// dX chain: transposed weights in one arithmetic (exact f32 image | split-bf16 stream | split-fp16 stream); every dZ section goes to
// `dz`; gscale (split-fp16 only): max |gradient| per dZ section, filled by the chain
typedef int (*NfChainLaunch)(const void* packed_t, const float* saved, const float* d_raw, int64_t n_points, float* dz, float* gscale,
                             nf_stream_t stream);

struct NfBwdFamily {
    int model;                        // index of the family's dW / reduce instantiations (k_dw_gemm_lds<M>, k_grad_reduce<M>, nfb_dw_plan)
    int64_t dz_per_point;             // floats of dZ sections per point
    int slab_floats;                  // floats of one partial-gradient slab
    int n_groups;                     // exact-f32 dW groups, filled by build_groups
    void (*build_groups)(NfDwGroup* groups);
    NfChainLaunch chain[3];           // exact f32 | split-bf16 | split-fp16
    void (*dw_f32)(const NfDwGroupSet& gset, const float* dz, const float* d_raw, const float* saved, int64_t n_points, float* slabs,
                   hipStream_t s);    // exact-f32 dW GEMMs (k_dw_gemm_lds<M>)
    void (*reduce_unpack)(const float* slabs, int n_slices, const NfReduceAlt& alt, float* sum, const float* packed, const float* cond,
                          float* grads, hipStream_t s);   // k_grad_reduce<M>, then the scatter into the reference-layout tensors
};

size_t nf_bwd_workspace_floats(const NfBwdFamily& fam, int64_t n_points);

// precision: 0 exact f32, 1 split-bf16, 2 split-fp16 (packed_t: the family's matching transposed image / stream).
// saved_f32 (split-bf16 chain only, else NULL): exact-f32 dW GEMMs on `saved` converted by nf_split_saved_to_f32.
// stage_ms (else NULL): synchronises and returns {dX chain, dW GEMMs, reduce + unpack} in milliseconds.
int nf_bwd_run(const NfBwdFamily& fam, int precision, const float* packed, const void* packed_t, const float* cond, const float* saved,
               const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads,
               nf_stream_t stream, float* stage_ms = nullptr, const float* saved_f32 = nullptr);
