/*
 * libnerface_hip.so -- C ABI of the MI355X (gfx950) implementation of NeRFace's ray-marching hot path.
 *
 * The reference (gafniguy/4D-Facial-Avatars) has no native/FFI layer: its boundary is the Python module
 * `nerf` (nerf/__init__.py:1-9).  Each entry point below replaces the stock-PyTorch op sequence of one
 * reference function; citations are relative to nerface_code/nerf-pytorch/ in the reference tree:
 *   H = nerf/nerf_helpers.py  V = nerf/volume_rendering_utils.py  T = nerf/train_utils.py  M = nerf/models.py
 *
 * Conventions: every pointer is a DEVICE pointer to contiguous row-major fp32 unless stated otherwise;
 * `stream` is a hipStream_t (NULL = default stream); kernels are enqueued asynchronously; the return
 * value is 0 on success or the hipError_t of the failed launch (nf_error_string() renders it), and
 * NF_EINVAL (-22) for an argument the library rejects.  No entry point allocates, frees or synchronises,
 * except nf_paper_pack's one-time upload of its (static) gather table and the first nf_paper_mlp_fwd_live
 * on a device, which allocates that device's unit counters.
 */
#ifndef NERFACE_HIP_H
#define NERFACE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nf_stream_t; /* hipStream_t */

#define NF_EINVAL (-22)

/* ---- library ------------------------------------------------------------------------------------ */
int         nf_abi_version(void);            /* bumped on any signature / layout change; now 5        */
const char* nf_error_string(int code);
const char* nf_build_info(void);             /* "gfx950 <compiler> <date>"                            */

/* ---- K1: ray generation  -- replaces get_ray_bundle (H:68-123, meshgrid_xy H:29-41) --------------- */
/* c2w: 3 rows x >=4 floats with row stride `c2w_row_stride`; cx_w = float(W*cx), cy_h = float(H*cy)
 * computed by the caller in double (H:111-114).  ro, rd: (H, W, 3).  Bit-exact with the reference.   */
int nf_ray_bundle(int height, int width, float fx, float fy, float cx_w, float cy_h,
                  const float* c2w, int c2w_row_stride, float* ro, float* rd, nf_stream_t stream);

/* K1 for a training batch -- replaces the full-frame get_ray_bundle plus the index gathers of one iteration
 * (train_transformed_rays.py:302, 325-330).  sel: (n, 2) int64 {row, col}, or with sel_is_flat (n) int64 pixel indices
 * row * width + col; ro, rd: (n, 3), bit-identical to rows of
 * nf_ray_bundle's output; target (n, channels) gathered from image (H, W, channels) and bg_out (n, 3) from bg (H, W, 3),
 * each optional (NULL).  bad_flag: one zeroed int on the device, set to 1 if a selected pixel lies outside the image.   */
int nf_ray_batch(int height, int width, float fx, float fy, float cx_w, float cy_h, const float* c2w, int c2w_row_stride,
                 const int64_t* sel, int sel_is_flat, int64_t n, const float* image, int channels, const float* bg, float* ro,
                 float* rd, float* target, float* bg_out, int* bad_flag, nf_stream_t stream);

/* ---- K0: ray selection of a training iteration -- replaces np.random.choice(H * W, size=n, replace=False, p=probs)
 *      (train_transformed_rays.py:320-322) -----------------------------------------------------------------------------
 * n_select DISTINCT indices in [0, n_items), drawn without replacement with probabilities proportional to weights (>= 0, need not
 * be normalised; items of weight 0 are never chosen).  u: n_items uniform numbers in [0, 1) from the caller's generator.
 * idx_out (n_select) int64, ascending for n_select <= 8192 (else in arbitrary order); entries stay -1, at the end (and word 5 of
 * the workspace is set), if fewer than n_select weights are positive.  workspace: nf_weighted_choice_workspace_bytes() bytes of device memory.                          */
size_t nf_weighted_choice_workspace_bytes(void);
int nf_weighted_choice(const float* weights, const float* u, int64_t n_items, int n_select, int64_t* idx_out, void* workspace,
                       size_t workspace_bytes, nf_stream_t stream);

/* ---- K2: stratified coarse depths -- replaces T:56-76 -------------------------------------------- */
/* z: (n_rays, n_coarse).  t_vals: (n_coarse) = the caller's torch.linspace(0,1,n_coarse) table (T:50-55;
 * passing the table keeps torch's own linspace rounding).  t_rand NULL => perturb off.  Bit-exact.    */
int nf_sample_coarse(int64_t n_rays, int n_coarse, float near_z, float far_z, const float* t_vals,
                     const float* t_rand, float* z, nf_stream_t stream);
/* same with the reference's `lindisp` switch (T:65-66): lindisp != 0 spaces the depths linearly in disparity,
 * z = 1 / (1/near (1 - t) + 1/far t).  Bit-exact.                                                       */
int nf_sample_coarse_ex(int64_t n_rays, int n_coarse, float near_z, float far_z, const float* t_vals,
                        const float* t_rand, int lindisp, float* z, nf_stream_t stream);

/* ---- K3: positional encoder -- replaces positional_encoding (H:195-239) --------------------------- */
/* x: (n_rows, dim) -> out: (n_rows, dim*(include_input + 2*n_freq)), layout [x | sin f0 | cos f0 | ..] */
int nf_posenc(const float* x, int64_t n_rows, int dim, int n_freq, int include_input, float* out,
              nf_stream_t stream);

/* ---- K4: fused MLP -- replaces run_network (T:9-33) + ConditionalBlendshapePaperNeRFModel.forward
 *      (M:236-261) including pts = ro + rd*z (T:78), both positional encodings and all concats ------ */
#define NF_PAPER_NUM_PARAMS 26   /* state_dict order: layers_xyz.{0..5}.{weight,bias}, fc_feat.*, fc_alpha.*,
                                    layers_dir.{0..3}.*, fc_rgb.*   (layers_dir.3 is dead weight, Q3)  */
size_t nf_paper_packed_floats(void);      /* size of the MFMA-fragment-ordered weight image           */
size_t nf_paper_cond_floats(void);        /* size of the per-call bias table                          */
/* Gather the 26 live nn.Parameter storages into the fragment-ordered image (re-run after each
 * optimizer step).  `params` is a HOST array of 26 device pointers.                                   */
int nf_paper_pack(const float* const* params, float* packed, nf_stream_t stream);
/* HOST copy of the gather table behind nf_paper_pack (layout tests without a GPU):
 * out[i] = (state_dict index << 24) | flat element offset, 0xFF000000 = constant zero.                 */
int nf_paper_gather_table(uint32_t* out, size_t n /* must equal nf_paper_packed_floats() */);
/* Fold the per-call constant input columns into bias vectors: expr*1/3 (76) and latent (32) into
 * layers_xyz.0 / layers_xyz.3 (M:239-246), PE4(near), PE4(far) into layers_dir.0 (Quirk Q1, T:14).    */
int nf_paper_condition(const float* packed, const float* expr76, const float* latent32,
                       float near_z, float far_z, float* cond, nf_stream_t stream);
/* raw[(ray*S + s)*4 + {0,1,2,3}] = (rgb_raw, sigma_raw) for points ro + rd*z[ray, s].                 */
/* rd_view: per-ray vector whose z component feeds the "direction" encoding (T:14); NULL = rd.  It differs
 * from rd only on the reference's ray-direction ablation path (T:81-82, Quirk Q7).                     */
int nf_paper_mlp_fwd(const float* packed, const float* cond, const float* ro, const float* rd,
                     const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,
                     nf_stream_t stream);

/* ---- ConditionalBlendshapePaperNeRFModel.forward on pre-encoded inputs (M:236-261 as run_network calls it, T:20-24):
 * x87 (n_points, 87) = [PE10(xyz) | PE4(dirs)], expr (76), latent (32) -> out (n_points, 4).  Inference; `cond` is scratch
 * of nf_paper_cond_floats() floats.  The hot path never builds x87 (nf_paper_mlp_fwd encodes in registers).            */
int nf_paper_forward_encoded(const float* packed, const float* x87, const float* expr76, const float* latent32,
                             int64_t n_points, float* cond, float* out, nf_stream_t stream);

/* ---- K4, split-bf16 variant (eval): every GEMM as 3 bf16 MFMAs (W_hi x_hi + W_hi x_lo + W_lo x_hi) with f32
 * accumulation -- ~2^-16 relative per layer instead of 2^-24, 3x the throughput of the exact-f32 matrix rate.
 * Same arguments/semantics as nf_paper_mlp_fwd; `cond` is the same table (from the f32 image).  north_star's 1e-4 dB gate
 * (profiles/r06_gate_sensitivity.md): held on whole frames against a uniform-random or a 20 dB target, marginal at a 30 dB
 * target on the x1000 density head (1.3e-4 dB), held everywhere on the x40 head; frames 75 .. 88 / 112 .. 124 dB from exact f32. */
size_t nf_paper_packed_bf16_bytes(void);
int nf_paper_pack_bf16(const float* const* params, void* packed_bf16, nf_stream_t stream);
int nf_paper_mlp_fwd_bf16(const void* packed_bf16, const float* cond, const float* ro, const float* rd,
                          const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,
                          nf_stream_t stream);

/* ---- K4, split-fp16 variant ("f16x3", csrc/nf_mlp_f16.hip): same contract as nf_paper_mlp_fwd, every product evaluated as
 * three fp16 MFMAs with f32 accumulation on a per-layer power-of-two-scaled weight stream: fp32-CLASS accuracy (22 operand
 * significand bits; measured error against fp64 at the exact-f32 kernel's level; whole frames AND small ray sets as close to the
 * exact-f32 frame as that frame is to a float64 evaluation, at every target: profiles/r06_gate_sensitivity.md) at the split-bf16
 * kernel's speed.
 * `packed_f16` = nf_paper_packed_f16_bytes() bytes from nf_paper_pack_f16 (stream blocks + per-layer scales).
 * Valid while |activations| < 4094 (fp16 range / 2^4); replaces M:236-261 like nf_paper_mlp_fwd.
 * Range guard: if an activation leaves fp16's range the point's outputs are non-finite and the kernel sets a sticky 32-bit
 * flag at byte nf_paper_f16_flag_offset() of `packed_f16` (cleared by nf_paper_pack_f16); callers poll it per frame.      */
size_t nf_paper_f16_flag_offset(void);
size_t nf_paper_packed_f16_bytes(void);
int nf_paper_pack_f16(const float* const* params, void* stream_out, nf_stream_t stream);
int nf_paper_mlp_fwd_f16(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                         const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
/* "f16x2" (round 5, csrc/nf_mlp_f16x2.hip): the same call on the same packed image with TWO fp16 products per weight -- activations enter
 * with their 11-bit `hi` half only, weights keep 22 bits: W_hi x_hi + W_lo x_hi, a third fewer MFMAs.  Inference only.  NOT an fp32-class
 * arithmetic: per-point outputs carry fp16's 2^-12 relative rounding of the activations, whole frames sit 60 .. 75 dB (x1000 density head) /
 * 85 .. 96 dB (x40 head) from the exact-f32 frame.  north_star's 1e-4 dB gate (round 6, profiles/r06_gate_sensitivity.md): held on whole
 * 512 x 512 frames against a uniform-random target (<= 5.6e-5 dB over 21 frames) and, on the x40 head, against targets the render approximates
 * to 20 .. 40 dB; MISSED against such targets on the x1000 head (4e-3 dB at 30 dB) and on ray sets of a few thousand rays.  Use
 * nf_paper_mlp_fwd_f16 where the gate must hold against real images; launch/eval_sharded.py measures it on the sequence being rendered.
 * Range and range guard as nf_paper_mlp_fwd_f16. */
int nf_paper_mlp_fwd_f16x2(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                           const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
/* training on the split-fp16 kernels ("f16x3": the three training GEMM kernels -- activation-saving forward, dX chain,
 * weight-gradient GEMMs -- at fp32-class accuracy on the 16-bit matrix pipe).  nf_paper_mlp_fwd_train_f16 fills `saved` like
 * nf_paper_mlp_fwd_train_bf16; nf_paper_mlp_bwd_f16 = nf_paper_mlp_bwd with the chain and the dW GEMMs on fp16 pairs, gradients
 * carried in block floating point (one power-of-two scale per point and layer; workspace as nf_paper_bwd_workspace_floats). */
int nf_paper_mlp_fwd_train_f16(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                               const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream);
size_t nf_paper_packed_bwd_f16_bytes(void);
int nf_paper_pack_bwd_f16(const float* const* params, void* stream_out, nf_stream_t stream);
int nf_paper_mlp_bwd_f16(const float* packed, const void* packed_t_f16, const float* cond, const float* saved, const float* d_raw,
                         int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads, nf_stream_t stream);
/* training forward on the split-bf16 kernel: also fills `saved` (f32, same layout as nf_paper_mlp_fwd_train); the
 * backward (nf_paper_mlp_bwd) stays on the exact-f32 kernels.                                                */
int nf_paper_mlp_fwd_train_bf16(const void* packed_bf16, const float* cond, const float* ro, const float* rd,
                                const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,
                                float* saved, nf_stream_t stream);

/* ---- K4 training path ---------------------------------------------------------------------------------
 * The reference trains through autograd (train_transformed_rays.py:389); here the forward saves every layer
 * output (`saved`, nf_paper_saved_floats(n_points) floats) and nf_paper_mlp_bwd turns d_raw (n_points,4)
 * into the gradients of all 26 parameters (reference layout, state_dict order, flattened) followed by the
 * 32 latent-code gradients: nf_paper_grad_floats() floats in total.  layers_dir.3 gets zeros (Quirk Q3).   */
size_t nf_paper_saved_floats(int64_t n_points);
int nf_paper_mlp_fwd_train(const float* packed, const float* cond, const float* ro, const float* rd,
                           const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,
                           float* saved, nf_stream_t stream);
size_t nf_paper_packed_bwd_floats(void);  /* transposed fragment image used by the backward chain        */
int nf_paper_pack_bwd(const float* const* params, float* packed_t, nf_stream_t stream);
size_t nf_paper_grad_floats(void);
size_t nf_paper_bwd_workspace_floats(int64_t n_points);
int nf_paper_mlp_bwd(const float* packed, const float* packed_t, const float* cond, const float* saved,
                     const float* d_raw, int64_t n_rays, int n_samples, float* workspace,
                     size_t workspace_floats, float* grads, nf_stream_t stream);

/* Measurement hook (bench.py's per-kernel training roofline; the reference has no counterpart): one backward in arithmetic
 * `precision` (0 exact f32, 1 split-bf16, 2 split-fp16; packed_t_any = the matching transposed image / stream) with HIP
 * events recorded on `stream` between its stages.  Synchronises the stream; stage_ms[3] (host) = {dX chain,
 * weight-gradient GEMMs, slab reduction + unpack} in milliseconds.                                                  */
int nf_paper_mlp_bwd_stage_ms(const float* packed, const void* packed_t_any, int precision, const float* cond,
                              const float* saved, const float* d_raw, int64_t n_rays, int n_samples, float* workspace,
                              size_t workspace_floats, float* grads, float* stage_ms, nf_stream_t stream);

/* Backward on the split-bf16 kernels: the dX chain and (unless exact_dw != 0) the weight-gradient GEMMs; bias/latent
 * reductions stay f32.  `saved` must have been written by nf_paper_mlp_fwd_train_bf16: the SPLIT TRAINING LAYOUT -- sections
 * n_points rounded up to 32 points long; every hidden layer's output as the weight-gradient kernel's (hi, lo) operand fragments
 * (csrc/nf_mlp_bf16_machinery.inc), positional encoding / dir slots as f32 rows, the ReLU bit masks the chain reads.
 * exact_dw != 0 runs the exact-f32 GEMMs instead; they read f32 rows: saved_f32 = `saved` converted by nf_split_saved_to_f32
 * (else NULL).
 * nf_split_saved_to_f32: model 0 paper / 1 second family; is_f16 = the forward was the split-fp16 one; out = nf_paper_saved_floats /
 * nf_lcode_saved_floats(n_points) floats in the exact-f32 training layout (x = hi + lo: 16 / 22 significand bits).        */
int nf_split_saved_to_f32(int model, const float* saved_split, int64_t n_points, int is_f16, float* out, nf_stream_t stream);
size_t nf_paper_packed_bwd_bf16_bytes(void);
int nf_paper_pack_bwd_bf16(const float* const* params, void* packed_t_bf16, nf_stream_t stream);
int nf_paper_mlp_bwd_bf16(const float* packed, const void* packed_t_bf16, const float* cond, const float* saved,
                          const float* d_raw, int64_t n_rays, int n_samples, float* workspace,
                          size_t workspace_floats, float* grads, int exact_dw, const float* saved_f32, nf_stream_t stream);

/* ---- K5: volume integrator -- replaces volume_render_radiance_field (V:7-75) + cumprod_exclusive
 *      (H:44-65) + the background overwrite of T:95-96 ----------------------------------------------- */
/* bg (n_rays,3) or NULL; noise (n_rays,S) already scaled by noise_std, or NULL.  Outputs: rgb (R,3),
 * disp (R), acc (R), weights (R,S).                                                                   */
int nf_volume_render_fwd(const float* raw, const float* z, const float* rd, const float* noise,
                         const float* bg, int64_t n_rays, int n_samples, int white_background,
                         float* rgb, float* disp, float* acc, float* weights, nf_stream_t stream);
/* d_raw (R,S,4) from d_rgb (R,3) (the trainer's loss only reaches rgb_map, TR:355-387).               */
int nf_volume_render_bwd(const float* raw, const float* z, const float* rd, const float* noise,
                         const float* bg, const float* d_rgb, int64_t n_rays, int n_samples,
                         int white_background, float* d_raw, nf_stream_t stream);
/* The full backward: a cotangent of every output, each optional (NULL = zero; all NULL is NF_EINVAL): d_rgb (R,3), d_disp (R),
 * d_acc (R), d_weights (R,S), and d_w_last (R), a cotangent of weights[:, -1] alone (so that no (R,S) tensor is needed for it).
 * d_bg (R,3) or NULL: the gradient of the background prior (= weights[:, -1] * d_rgb; needs bg).  Same limits as
 * nf_volume_render_bwd, which stays the path of a backward that carries d_rgb only.                    */
int nf_volume_render_bwd_full(const float* raw, const float* z, const float* rd, const float* noise,
                              const float* bg, const float* d_rgb, const float* d_disp, const float* d_acc,
                              const float* d_weights, const float* d_w_last, int64_t n_rays, int n_samples,
                              int white_background, float* d_raw, float* d_bg, nf_stream_t stream);

/* ---- second model family: ConditionalBlendshapeLearnableCodeNeRFModel.forward (M:590-636) + run_network (T:9-33), inference.
 * params: HOST array of 16 device pointers in state_dict order (layer1, layers_xyz.0..2, layers_dir.0, fc_alpha, fc_rgb,
 * fc_feat; weight then bias).  Same pack / condition / forward protocol and argument meaning as the paper model.      */
size_t nf_lcode_packed_floats(void);
size_t nf_lcode_cond_floats(void);
int nf_lcode_pack(const float* const* params, float* packed, nf_stream_t stream);
int nf_lcode_condition(const float* packed, const float* expr76, const float* latent32, float near_z, float far_z,
                       float* cond, nf_stream_t stream);
int nf_lcode_mlp_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                     const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
/* ConditionalBlendshapeLearnableCodeNeRFModel.forward on PRE-ENCODED inputs (replaces M:590-636 as run_network calls it, T:9-33):
 * x87 (n_points, 87) = [PE10(xyz) | PE4(dirs)] -> out (n_points, 4); `cond` = scratch of nf_lcode_cond_floats() floats.  Inference
 * only (ABI 4); the hot path never materialises x87 and uses nf_lcode_mlp_fwd. */
int nf_lcode_forward_encoded(const float* packed, const float* x87, const float* expr76, const float* latent32,
                             int64_t n_points, float* cond, float* out, nf_stream_t stream);
/* The same inference forward in split-bf16 arithmetic (see nf_paper_mlp_fwd_bf16): stream of
 * nf_lcode_packed_bf16_bytes() bytes packed from the same 16 tensors; `cond` as filled by nf_lcode_condition.          */
size_t nf_lcode_packed_bf16_bytes(void);
int nf_lcode_pack_bf16(const float* const* params, void* packed_bf16, nf_stream_t stream);
int nf_lcode_mlp_fwd_bf16(const void* packed_bf16, const float* cond, const float* ro, const float* rd,
                          const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,
                          nf_stream_t stream);
/* split-fp16 ("f16x3") forward of the second model family: contract, valid range and range guard as nf_paper_mlp_fwd_f16 */
size_t nf_lcode_packed_f16_bytes(void);
size_t nf_lcode_f16_flag_offset(void);
int nf_lcode_pack_f16(const float* const* params, void* stream_out, nf_stream_t stream);
int nf_lcode_mlp_fwd_f16(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                         const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
int nf_lcode_mlp_fwd_f16x2(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                           const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);   /* "f16x2": see nf_paper_mlp_fwd_f16x2 */
/* training the second family on the split-fp16 kernels (as nf_paper_mlp_fwd_train_f16 / nf_paper_mlp_bwd_f16) */
int nf_lcode_mlp_fwd_train_f16(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                               const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream);
size_t nf_lcode_packed_bwd_f16_bytes(void);
int nf_lcode_pack_bwd_f16(const float* const* params, void* stream_out, nf_stream_t stream);
int nf_lcode_mlp_bwd_f16(const float* packed, const void* packed_t_f16, const float* cond, const float* saved, const float* d_raw,
                         int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads, nf_stream_t stream);

/* Training of the same family, exact f32 (autograd through M:590-636 as the trainer drives it, TR:355-392):
 * forward that also fills `saved` (nf_lcode_saved_floats(n_rays*n_samples) floats), transposed weight image, and the
 * backward: grads = the 16 tensors in the order of nerf.models.LCODE_KEYS (layer1, layers_xyz.0..2, layers_dir.0,
 * fc_alpha, fc_rgb, fc_feat; weight then bias), flattened, followed by d latent (32).                                */
size_t nf_lcode_saved_floats(int64_t n_points);
int nf_lcode_mlp_fwd_train(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                           const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream);
size_t nf_lcode_packed_bwd_floats(void);
int nf_lcode_pack_bwd(const float* const* params, float* packed_t, nf_stream_t stream);
size_t nf_lcode_grad_floats(void);
size_t nf_lcode_bwd_workspace_floats(int64_t n_points);
int nf_lcode_mlp_bwd(const float* packed, const float* packed_t, const float* cond, const float* saved, const float* d_raw,
                     int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads,
                     nf_stream_t stream);

/* Training of the same family on the split-bf16 kernels (forward, dX chain, weight-gradient GEMMs; reductions f32).   */
int nf_lcode_mlp_fwd_train_bf16(const void* packed_bf16, const float* cond, const float* ro, const float* rd,
                                const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw,
                                float* saved, nf_stream_t stream);
size_t nf_lcode_packed_bwd_bf16_bytes(void);
int nf_lcode_pack_bwd_bf16(const float* const* params, void* packed_t_bf16, nf_stream_t stream);
int nf_lcode_mlp_bwd_bf16(const float* packed, const void* packed_t_bf16, const float* cond, const float* saved,
                          const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                          float* grads, nf_stream_t stream);

/* ---- the two blendshape classes without a learnable code, on the second family's per-point kernels (additive to ABI 5) ----------
 * nf_bshape_*:  ConditionalBlendshapeNeRFModel (M:872-976): layer1 reads [PE 63 | expr/3 76].  params: HOST array of 16 device
 *               pointers, the second family's order, layer1.weight (256, 139).
 * nf_cbshape_*: ConditionalCompressedBlendshapeNeRFModel (M:750-868): layer1 reads [PE 63 | e3 20], e3 = the expression encoder
 *               layers_expr (76 -> 38 -> 20 -> 20, a ReLU after each layer, expression not divided by 3), evaluated once per call by
 *               nf_cbshape_condition.  params: HOST array of 22 device pointers in state_dict order (layers_expr.0..2, then the 16 of
 *               the second family with layer1.weight (256, 83)); its packed f32 image carries the encoder behind the trunk image.
 * Every entry point has the signature and the argument meaning of its nf_lcode_* namesake; images, `cond`, `saved` and the
 * workspace have the second family's sizes (nf_cbshape_packed_floats() excepted).  latent32 is accepted and ignored (may be NULL).
 * grads: the class's tensors in params order, flattened, then 32 zeros (d latent: neither class reads a latent code).            */
size_t nf_bshape_packed_floats(void);
size_t nf_bshape_cond_floats(void);
int nf_bshape_pack(const float* const* params, float* packed, nf_stream_t stream);
int nf_bshape_condition(const float* packed, const float* expr76, const float* latent32, float near_z, float far_z, float* cond,
                    nf_stream_t stream);
int nf_bshape_mlp_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view, const float* z,
                  int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
int nf_bshape_forward_encoded(const float* packed, const float* x87, const float* expr76, const float* latent32, int64_t n_points,
                          float* cond, float* out, nf_stream_t stream);
size_t nf_bshape_packed_bf16_bytes(void);
int nf_bshape_pack_bf16(const float* const* params, void* packed_bf16, nf_stream_t stream);
int nf_bshape_mlp_fwd_bf16(const void* packed_bf16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                       const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
size_t nf_bshape_packed_f16_bytes(void);
size_t nf_bshape_f16_flag_offset(void);
int nf_bshape_pack_f16(const float* const* params, void* stream_out, nf_stream_t stream);
int nf_bshape_mlp_fwd_f16(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                      const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
int nf_bshape_mlp_fwd_f16x2(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                        const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
size_t nf_bshape_saved_floats(int64_t n_points);
int nf_bshape_mlp_fwd_train(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                        const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream);
int nf_bshape_mlp_fwd_train_bf16(const void* packed_bf16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                             const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream);
int nf_bshape_mlp_fwd_train_f16(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                            const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream);
size_t nf_bshape_packed_bwd_floats(void);
int nf_bshape_pack_bwd(const float* const* params, float* packed_t, nf_stream_t stream);
size_t nf_bshape_packed_bwd_bf16_bytes(void);
int nf_bshape_pack_bwd_bf16(const float* const* params, void* packed_t_bf16, nf_stream_t stream);
size_t nf_bshape_packed_bwd_f16_bytes(void);
int nf_bshape_pack_bwd_f16(const float* const* params, void* stream_out, nf_stream_t stream);
size_t nf_bshape_grad_floats(void);
size_t nf_bshape_bwd_workspace_floats(int64_t n_points);
int nf_bshape_mlp_bwd(const float* packed, const float* packed_t, const float* cond, const float* saved, const float* d_raw,
                  int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads, nf_stream_t stream);
int nf_bshape_mlp_bwd_bf16(const float* packed, const void* packed_t_bf16, const float* cond, const float* saved, const float* d_raw,
                       int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads, nf_stream_t stream);
int nf_bshape_mlp_bwd_f16(const float* packed, const void* packed_t_f16, const float* cond, const float* saved, const float* d_raw,
                      int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads, nf_stream_t stream);

size_t nf_cbshape_packed_floats(void);
size_t nf_cbshape_cond_floats(void);
int nf_cbshape_pack(const float* const* params, float* packed, nf_stream_t stream);
int nf_cbshape_condition(const float* packed, const float* expr76, const float* latent32, float near_z, float far_z, float* cond,
                    nf_stream_t stream);
int nf_cbshape_mlp_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view, const float* z,
                  int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
int nf_cbshape_forward_encoded(const float* packed, const float* x87, const float* expr76, const float* latent32, int64_t n_points,
                          float* cond, float* out, nf_stream_t stream);
size_t nf_cbshape_packed_bf16_bytes(void);
int nf_cbshape_pack_bf16(const float* const* params, void* packed_bf16, nf_stream_t stream);
int nf_cbshape_mlp_fwd_bf16(const void* packed_bf16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                       const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
size_t nf_cbshape_packed_f16_bytes(void);
size_t nf_cbshape_f16_flag_offset(void);
int nf_cbshape_pack_f16(const float* const* params, void* stream_out, nf_stream_t stream);
int nf_cbshape_mlp_fwd_f16(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                      const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
int nf_cbshape_mlp_fwd_f16x2(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                        const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
size_t nf_cbshape_saved_floats(int64_t n_points);
int nf_cbshape_mlp_fwd_train(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                        const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream);
int nf_cbshape_mlp_fwd_train_bf16(const void* packed_bf16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                             const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream);
int nf_cbshape_mlp_fwd_train_f16(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,
                            const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream);
size_t nf_cbshape_packed_bwd_floats(void);
int nf_cbshape_pack_bwd(const float* const* params, float* packed_t, nf_stream_t stream);
size_t nf_cbshape_packed_bwd_bf16_bytes(void);
int nf_cbshape_pack_bwd_bf16(const float* const* params, void* packed_t_bf16, nf_stream_t stream);
size_t nf_cbshape_packed_bwd_f16_bytes(void);
int nf_cbshape_pack_bwd_f16(const float* const* params, void* stream_out, nf_stream_t stream);
size_t nf_cbshape_grad_floats(void);
size_t nf_cbshape_bwd_workspace_floats(int64_t n_points);
int nf_cbshape_mlp_bwd(const float* packed, const float* packed_t, const float* cond, const float* saved, const float* d_raw,
                  int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads, nf_stream_t stream);
int nf_cbshape_mlp_bwd_bf16(const float* packed, const void* packed_t_bf16, const float* cond, const float* saved, const float* d_raw,
                       int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads, nf_stream_t stream);
int nf_cbshape_mlp_bwd_f16(const float* packed, const void* packed_t_f16, const float* cond, const float* saved, const float* d_raw,
                      int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads, nf_stream_t stream);

/* Measurement hook (tools/time_blendshape.py): nf_paper_mlp_bwd_stage_ms for the second family and the two classes on its kernels --
 * one backward in arithmetic `precision` (0 exact f32 | 1 split-bf16 | 2 split-fp16; packed_t_any: the matching transposed image) with
 * HIP events between its stages; synchronises the stream; stage_ms[3] (host) = {dX chain, weight-gradient GEMMs, reduce + scatter}.  */
int nf_lcode_mlp_bwd_stage_ms(const float* packed, const void* packed_t_any, int precision, const float* cond, const float* saved,
                              const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                              float* grads, float* stage_ms, nf_stream_t stream);
int nf_bshape_mlp_bwd_stage_ms(const float* packed, const void* packed_t_any, int precision, const float* cond, const float* saved,
                               const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                               float* grads, float* stage_ms, nf_stream_t stream);
int nf_cbshape_mlp_bwd_stage_ms(const float* packed, const void* packed_t_any, int precision, const float* cond, const float* saved,
                                const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                float* grads, float* stage_ms, nf_stream_t stream);

/* ---- third model family: ConditionalBlendshapePaperSmallerNeRFModel (M:266-338) + run_network (T:9-33) -- the paper model without
 * layers_xyz.5 and layers_dir.3, with layers_dir.0 reading [feat 256 | PE4(dir) 24 | expr/3 76].  EXACT F32 ONLY (no split
 * arithmetics).  params: HOST array of 22 device pointers in state_dict order (layers_xyz.0..4, fc_feat, fc_alpha, layers_dir.0..2,
 * fc_rgb; weight then bias).  Every nf_smaller_* entry point has the signature and the argument meaning of its nf_paper_*
 * namesake; additive to ABI 5.  nf_smaller_condition also folds the 76 expression columns of layers_dir.0 into its bias.
 * grads (nf_smaller_grad_floats()): the 22 tensors in state_dict order, flattened, then d latent (32); no tensor is dead.      */
size_t nf_smaller_packed_floats(void);
size_t nf_smaller_cond_floats(void);
int nf_smaller_gather_table(uint32_t* out, size_t n /* must equal nf_smaller_packed_floats() */);
int nf_smaller_pack(const float* const* params, float* packed, nf_stream_t stream);
int nf_smaller_condition(const float* packed, const float* expr76, const float* latent32, float near_z, float far_z,
                         float* cond, nf_stream_t stream);
int nf_smaller_mlp_fwd(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                       const float* z, int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
int nf_smaller_forward_encoded(const float* packed, const float* x87, const float* expr76, const float* latent32,
                               int64_t n_points, float* cond, float* out, nf_stream_t stream);
size_t nf_smaller_saved_floats(int64_t n_points);
int nf_smaller_mlp_fwd_train(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                             const float* z, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream);
size_t nf_smaller_packed_bwd_floats(void);
int nf_smaller_pack_bwd(const float* const* params, float* packed_t, nf_stream_t stream);
size_t nf_smaller_grad_floats(void);
size_t nf_smaller_bwd_workspace_floats(int64_t n_points);
int nf_smaller_mlp_bwd(const float* packed, const float* packed_t, const float* cond, const float* saved, const float* d_raw,
                       int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats, float* grads,
                       nf_stream_t stream);
/* Measurement hook (tools/time_smaller.py): one exact-f32 backward with HIP events between its stages; synchronises the stream;
 * stage_ms[3] (host) = {dX chain, weight-gradient GEMMs, slab reduction + unpack} in milliseconds.                           */
int nf_smaller_mlp_bwd_stage_ms(const float* packed, const float* packed_t, const float* cond, const float* saved,
                                const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                float* grads, float* stage_ms, nf_stream_t stream);

/* ---- BASELINE config 1: tiny_nerf.py (reference tiny_nerf.py:12-181) ----------------------------------------------
 * nf_tiny_mlp_fwd = compute_query_points_from_rays' pts = ro + rd*depth (tiny_nerf.py:59-63) + positional_encoding(., 10)
 * + VeryTinyNerfModel.forward (63 -> 128 -> 128 -> 4).  params: HOST array of 6 device pointers
 * (layer1.weight, layer1.bias, layer2.*, layer3.*).  depth: (n_rays, n_samples) if depth_per_ray else (n_samples).
 * nf_render_volume_density = render_volume_density (tiny_nerf.py:68-107) -> rgb (R,3), depth_map (R), acc (R).     */
size_t nf_tiny_packed_floats(void);
int nf_tiny_pack(const float* const* params, float* packed, nf_stream_t stream);
int nf_tiny_mlp_fwd(const float* packed, const float* ro, const float* rd, const float* depth, int depth_per_ray,
                    int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
int nf_render_volume_density(const float* raw, const float* depth, int64_t n_rays, int n_samples, float* rgb,
                             float* depth_map, float* acc, nf_stream_t stream);

/* ---- training the tiny path: autograd of run_one_iter_of_tinynerf (tiny_nerf.py:111-159) under the trainer's rgb loss
 *      (tiny_nerf.py:291-302), exact f32.  nf_tiny_mlp_fwd_train also writes the activations the backward needs (`saved`,
 *      nf_tiny_saved_floats(n_points) floats); nf_render_volume_density_bwd turns d loss / d rgb (R,3) into d_raw (R,S,4);
 *      nf_tiny_mlp_bwd turns d_raw into the six parameter gradients, concatenated in state_dict order
 *      [layer1.weight (128,63) | layer1.bias | layer2.weight | layer2.bias | layer3.weight (4,128) | layer3.bias]
 *      (nf_tiny_grad_floats() floats).  packed_t = nf_tiny_pack_bwd (transposed fragment image of layer2 / layer3).       */
size_t nf_tiny_saved_floats(int64_t n_points);
int nf_tiny_mlp_fwd_train(const float* packed, const float* ro, const float* rd, const float* depth, int depth_per_ray,
                          int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream);
int nf_render_volume_density_bwd(const float* raw, const float* depth, const float* d_rgb, int64_t n_rays, int n_samples,
                                 float* d_raw, nf_stream_t stream);
/* the same through all three outputs (rgb_map, depth_map, acc_map); each cotangent optional, all NULL is NF_EINVAL */
int nf_render_volume_density_bwd_full(const float* raw, const float* depth, const float* d_rgb, const float* d_depth,
                                      const float* d_acc, int64_t n_rays, int n_samples, float* d_raw, nf_stream_t stream);
size_t nf_tiny_packed_bwd_floats(void);
int nf_tiny_pack_bwd(const float* const* params, float* packed_t, nf_stream_t stream);
size_t nf_tiny_grad_floats(void);
size_t nf_tiny_bwd_workspace_floats(int64_t n_points);
int nf_tiny_mlp_bwd(const float* packed_t, const float* saved, const float* d_raw, int64_t n_rays, int n_samples,
                    float* workspace, size_t workspace_floats, float* grads, nf_stream_t stream);

/* ---- BASELINE config 1 read literally ("4-layer MLP"): the tiny path with the reference's FlexibleNeRFModel
 *      (nerf/models.py:351-422) constructed as FlexibleNeRFModel(num_layers = L, hidden_size = 128, num_encoding_fn_xyz = 10,
 *      include_input_xyz = True, use_viewdirs = False), L = 2 .. 5 (ABI 5):
 *        PE(63) -> layer1 (Linear 128, no activation, models.py:402) -> (L - 1) x [layers_xyz.k: Linear 128 + ReLU, models.py:403-410]
 *        -> fc_out (Linear 4, models.py:422).
 *      The entry points mirror nf_tiny_* with num_layers in front (other values: NF_EINVAL / size 0).  params: HOST array of
 *      4 + 2 (L - 1) device pointers in state_dict order (layer1.weight, layer1.bias, layers_xyz.0.weight, layers_xyz.0.bias, ...,
 *      fc_out.weight, fc_out.bias); nf_flex_mlp_bwd returns the gradients concatenated in the same order
 *      (nf_flex_grad_floats(L) floats).  Compositing: nf_render_volume_density(_bwd), as for the tiny path.                    */
size_t nf_flex_packed_floats(int num_layers);
int nf_flex_pack(int num_layers, const float* const* params, float* packed, nf_stream_t stream);
int nf_flex_mlp_fwd(int num_layers, const float* packed, const float* ro, const float* rd, const float* depth, int depth_per_ray,
                    int64_t n_rays, int n_samples, float* raw, nf_stream_t stream);
size_t nf_flex_saved_floats(int num_layers, int64_t n_points);
int nf_flex_mlp_fwd_train(int num_layers, const float* packed, const float* ro, const float* rd, const float* depth,     /* < 2^22 points */
                          int depth_per_ray, int64_t n_rays, int n_samples, float* raw, float* saved, nf_stream_t stream);
size_t nf_flex_packed_bwd_floats(int num_layers);
int nf_flex_pack_bwd(int num_layers, const float* const* params, float* packed_t, nf_stream_t stream);
size_t nf_flex_grad_floats(int num_layers);
size_t nf_flex_bwd_workspace_floats(int num_layers, int64_t n_points);
int nf_flex_mlp_bwd(int num_layers, const float* packed_t, const float* saved, const float* d_raw, int64_t n_rays, int n_samples,
                    float* workspace, size_t workspace_floats, float* grads, nf_stream_t stream);

/* ---- eval post-processing on the device -- replaces cast_to_image (eval_transformed_rays.py:184-190) and
 *      torch_normal_map(depthmap, focal, weights, clean=True) (eval_transformed_rays.py:84-119) ------------------------
 * rgb (H,W,3) -> rgb_u8 (H,W,3) = uint8(clamp(x,0,1)*255);  depthmap (H,W) [+ weights (H,W)] -> normals_u8 (H-1,W-1,3).
 * Either output may be NULL.  cx_w = cx*W, cy_h = cy*H as in nf_ray_bundle.                                              */
int nf_eval_postprocess(const float* rgb, const float* depthmap, const float* weights, int height, int width, float fx,
                        float fy, float cx_w, float cy_h, uint8_t* rgb_u8, uint8_t* normals_u8, nf_stream_t stream);

/* ---- image metrics of rendered frames -- replaces what nerf/metrics.py (two_folders) takes from skimage: L1, compare_psnr and
 *      compare_ssim(im1, im2, multichannel=True) of float images byte / 255, for n image pairs in one launch -------------------
 * a, b: uint8 [n][H][W][3], contiguous (a = rendered frame, b = test image).  out_f64 [n][4] = {L1 = mean |a - b| / 255,
 * MSE = mean ((a - b) / 255)^2, PSNR = 10 log10(1 / MSE) (+inf for identical images), SSIM}; out_i64 [n][2] = {sum |a - b|,
 * sum (a - b)^2} in byte units.  SSIM: 7 x 7 uniform window, sample covariance, C1 = (0.01 R)^2, C2 = (0.03 R)^2 with
 * R = ssim_range, mean over the windows inside the image and the channels; window statistics are exact integers, S is evaluated in
 * float64.  R = 2.0 reproduces the reference (that skimage takes the float dtype's range (-1, 1)); 1.0 is the textbook value.
 * Results are bit-identical from run to run (fixed-order reduction through `workspace`, no floating-point atomics).
 * NF_EINVAL: NULL pointers, H < 7, W < 7, n < 0, workspace_bytes below nf_image_metrics_workspace_bytes(n, H, W); n == 0: no launch. */
size_t nf_image_metrics_workspace_bytes(int64_t n, int height, int width);
int nf_image_metrics(const uint8_t* a, const uint8_t* b, int64_t n, int height, int width, double ssim_range, void* workspace,
                     size_t workspace_bytes, double* out_f64, int64_t* out_i64, nf_stream_t stream);

/* ---- K6: inverse-CDF sampler -- replaces sample_pdf_2 (H:344-387) --------------------------------- */
/* bins (R,n_bins), weights (R,n_bins-1); u: row r at u + r*u_row_stride, n_out values
 * (u_row_stride = n_out for torch.rand draws, 0 to broadcast the det-mode linspace(0,1,n_out) table). */
int nf_sample_pdf(const float* bins, const float* weights, const float* u, int64_t u_row_stride,
                  int64_t n_rays, int n_bins, int n_out, float* samples, nf_stream_t stream);
/* The CDF table is bit-identical to torch-CPU's (float row sum in ATen's 8-lane / 4-way-ILP order, sequential double
 * cumsum rounded per element), so the searchsorted indices equal the reference's.  The _ex form also returns them:
 * inds (R,n_out) int32 = torch.searchsorted(cdf, u, right=True) (H:368), cdf (R,n_bins); either may be NULL.           */
int nf_sample_pdf_ex(const float* bins, const float* weights, const float* u, int64_t u_row_stride, int64_t n_rays,
                     int n_bins, int n_out, float* samples, int* inds, float* cdf, nf_stream_t stream);

/* ---- K6+K7 fused: hierarchical resampling -- replaces T:116-126 (z_mid, sample_pdf on w[1:-1],
 *      sort(cat(z, z_samples))) ---------------------------------------------------------------------- */
int nf_resample_merge(const float* z_coarse, const float* w_coarse, const float* u, int64_t u_row_stride,
                      int64_t n_rays, int n_coarse, int n_fine, float* z_samples /* (R,n_fine) or NULL */,
                      float* z_fine /* (R,n_coarse+n_fine) */, nf_stream_t stream);

/* ---- whole per-chunk inference pipeline -- replaces predict_and_render_radiance (T:36-162) in eval: coarse depths,
 *      coarse MLP, integrator, resampling, fine MLP, integrator, 7-tuple (T:162), paper model.  One call, caller-provided
 *      workspace (nf_render_rays_workspace_floats), kernels enqueued on `stream`.  packed_bf16_* non-NULL selects the
 *      split-bf16 MLP kernel for that network.  n_fine = 0: coarse only (fine outputs untouched, w_last from the coarse pass).
 *      t_vals: linspace(0,1,n_coarse) table; t_rand / noise_* NULL = off; u as in nf_sample_pdf.                         */
size_t nf_render_rays_workspace_floats(int64_t n_rays, int n_coarse, int n_fine);
int nf_render_rays_fwd(const float* packed_coarse, const void* packed_bf16_coarse, const float* packed_fine,
                       const void* packed_bf16_fine, const float* expr76, const float* latent32, const float* ro,
                       const float* rd, const float* rd_view, const float* bg, const float* t_vals, const float* t_rand,
                       const float* u, int64_t u_row_stride, const float* noise_coarse, const float* noise_fine,
                       int64_t n_rays, int n_coarse, int n_fine, float near_z, float far_z, int white_background,
                       float* workspace, size_t workspace_floats, float* rgb_coarse, float* disp_coarse, float* acc_coarse,
                       float* rgb_fine, float* disp_fine, float* acc_fine, float* w_last, nf_stream_t stream);

/* The same pipeline with the split-fp16 MLP kernels: packed_f16_* = streams of nf_paper_pack_f16 (NULL: that network runs exact f32). */
int nf_render_rays_fwd_f16(const float* packed_coarse, const void* packed_f16_coarse, const float* packed_fine,
                           const void* packed_f16_fine, const float* expr76, const float* latent32, const float* ro,
                           const float* rd, const float* rd_view, const float* bg, const float* t_vals, const float* t_rand,
                           const float* u, int64_t u_row_stride, const float* noise_coarse, const float* noise_fine,
                           int64_t n_rays, int n_coarse, int n_fine, float near_z, float far_z, int white_background,
                           float* workspace, size_t workspace_floats, float* rgb_coarse, float* disp_coarse, float* acc_coarse,
                           float* rgb_fine, float* disp_fine, float* acc_fine, float* w_last, nf_stream_t stream);

/* ... and with two fp16 products per weight ("f16x2", nf_paper_mlp_fwd_f16x2): the same streams, the same arguments. */
int nf_render_rays_fwd_f16x2(const float* packed_coarse, const void* packed_f16_coarse, const float* packed_fine,
                             const void* packed_f16_fine, const float* expr76, const float* latent32, const float* ro,
                             const float* rd, const float* rd_view, const float* bg, const float* t_vals, const float* t_rand,
                             const float* u, int64_t u_row_stride, const float* noise_coarse, const float* noise_fine,
                             int64_t n_rays, int n_coarse, int n_fine, float near_z, float far_z, int white_background,
                             float* workspace, size_t workspace_floats, float* rgb_coarse, float* disp_coarse, float* acc_coarse,
                             float* rgb_fine, float* disp_fine, float* acc_fine, float* w_last, nf_stream_t stream);

/* ---- optimizer step of the trainer -- replaces torch.optim.Adam.step() over [coarse model, fine model, latent codes]
 *      (train_transformed_rays.py:193-199, 391-392) for all tensors in one launch.  Host arrays of n_tensors device pointers
 *      (contiguous f32, numel[i] elements each); step = 1-based count of this update; torch's arithmetic (no weight decay,
 *      no amsgrad): m += (1-b1)(g-m); v = b2 v + (1-b2) g g; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).            */
int nf_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                 const int64_t* numel, int n_tensors, float lr, float beta1, float beta2, float eps, int64_t step,
                 nf_stream_t stream);

/* ---- the trainer's loss and its gradients -- replaces TR:355-387 (coarse = mse_loss(rgb_coarse, target); fine = mse_loss(rgb_fine,
 *      target); code = code_weight * torch.norm(latent); loss = coarse + fine + code_scale * code) and the backward of those nodes
 *      (~20 torch launches) by two launches.  n_elems = numel of the colour maps (contiguous f32, same shape as target); rgb_fine and
 *      latent may be NULL.  out7 = {loss, coarse mse, fine mse, code loss, coarse + fine, -10 log10(coarse + fine), ||latent||}.
 *      Backward: grad_out = device scalar d(loss); d_rgb = ((2 / n)(rgb - target)) * grad_out (ATen's mse_loss_backward),
 *      d_latent = latent * (grad_out * code_scale * code_weight / ||latent||), 0 at a zero norm (ATen's norm_backward).            */
int nf_train_loss_fwd(const float* rgb_coarse, const float* rgb_fine, const float* target, int64_t n_elems, const float* latent,
                      int n_latent, float code_weight, float code_scale, float* out7, nf_stream_t stream);
int nf_train_loss_bwd(const float* rgb_coarse, const float* rgb_fine, const float* target, int64_t n_elems, const float* latent,
                      int n_latent, float code_weight, float code_scale, const float* out7, const float* grad_out,
                      float* d_rgb_coarse, float* d_rgb_fine, float* d_latent, nf_stream_t stream);

/* ---- the same two pieces in the form a captured HIP graph can replay (additive to ABI 5) ---------------------------------------
 * nf_adam_step_dev: nf_adam_step with the step count and the learning-rate schedule in a device block the caller owns, instead of
 *      host scalars (kernel arguments are frozen in a captured graph).  state: 32 bytes, 8-byte aligned:
 *        { float step (completed steps); int32 ticket (0 between launches); double lr0, decay_factor, decay_steps }.
 *      Step i = `step` before the launch runs with lr = i == 0 ? lr0 : lr0 * decay_factor ^ ((i - 1) / decay_steps) (the lr the
 *      trainer set at the end of step i - 1, TR:395-400; double, rounded to f32 once) and bias corrections of t = i + 1 in
 *      nf_adam_step's operation order; the launch leaves step = i + 1 (one thread stores it after every workgroup has read i).
 * nf_train_loss_bg_*: nf_train_loss_* plus the trainer's background-supervision term (TR:376-381)
 *        bg_loss = mean_r(sum_c (bg[r, c] - target[r, c])^2 * w_last[r]) * bg_weight
 *      n_elems = 3 n_rays (colour maps, target, bg: (n_rays, 3) contiguous f32; w_last: (n_rays)).  out8 = out7 with the term added
 *      to out8[0], and out8[7] = bg_loss.  Backward: also d_bg (n_rays, 3) and d_w_last (n_rays).                                */
int nf_adam_step_dev(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                     const int64_t* numel, int n_tensors, float beta1, float beta2, float eps, void* state, nf_stream_t stream);
int nf_train_loss_bg_fwd(const float* rgb_coarse, const float* rgb_fine, const float* target, int64_t n_elems, const float* latent,
                         int n_latent, float code_weight, float code_scale, const float* bg, const float* w_last, float bg_weight,
                         float* out8, nf_stream_t stream);
int nf_train_loss_bg_bwd(const float* rgb_coarse, const float* rgb_fine, const float* target, int64_t n_elems, const float* latent,
                         int n_latent, float code_weight, float code_scale, const float* bg, const float* w_last, float bg_weight,
                         const float* out8, const float* grad_out, float* d_rgb_coarse, float* d_rgb_fine, float* d_latent,
                         float* d_bg, float* d_w_last, nf_stream_t stream);

/* ---- K7: per-ray ascending sort -- replaces torch.sort(...)[0] at T:126 --------------------------- */
int nf_sort_rows(const float* in, int64_t n_rows, int n_cols, float* out, nf_stream_t stream);

/* ---- density only (ABI 5 still: these only add) -----------------------------------------------------------------------------
 * <prefix>_mlp_sigma*: the inference forward <prefix>_mlp_fwd* up to and including the layer that yields the raw density, and
 * nothing after it: sigma[n_rays * n_samples] = raw[..., 3] of the full forward (before the ReLU), the same operations in the same
 * order.  Arguments, images, bias table, NF_EINVAL / zero-ray conventions, valid range and range guard as the full forward of the
 * same arithmetic; rd_view is accepted and not read by the exact-f32 kernels (the direction never reaches fc_alpha).  The smaller
 * paper model has the exact-f32 form only, like its forward.                                                                   */
#define NF_DECLARE_MLP_SIGMA(PFX)                                                                                                   \
    int PFX##_mlp_sigma(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,            \
                        const float* z, int64_t n_rays, int n_samples, float* sigma, nf_stream_t stream);
#define NF_DECLARE_MLP_SIGMA_SPLIT(PFX)                                                                                             \
    int PFX##_mlp_sigma_bf16(const void* packed_bf16, const float* cond, const float* ro, const float* rd, const float* rd_view,   \
                             const float* z, int64_t n_rays, int n_samples, float* sigma, nf_stream_t stream);                     \
    int PFX##_mlp_sigma_f16(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,     \
                            const float* z, int64_t n_rays, int n_samples, float* sigma, nf_stream_t stream);                      \
    int PFX##_mlp_sigma_f16x2(const void* packed_f16, const float* cond, const float* ro, const float* rd, const float* rd_view,   \
                              const float* z, int64_t n_rays, int n_samples, float* sigma, nf_stream_t stream);
NF_DECLARE_MLP_SIGMA(nf_paper) NF_DECLARE_MLP_SIGMA_SPLIT(nf_paper)       /* nf_paper_mlp_sigma, _sigma_bf16, _sigma_f16, _sigma_f16x2 */
NF_DECLARE_MLP_SIGMA(nf_lcode) NF_DECLARE_MLP_SIGMA_SPLIT(nf_lcode)
NF_DECLARE_MLP_SIGMA(nf_bshape) NF_DECLARE_MLP_SIGMA_SPLIT(nf_bshape)
NF_DECLARE_MLP_SIGMA(nf_cbshape) NF_DECLARE_MLP_SIGMA_SPLIT(nf_cbshape)
NF_DECLARE_MLP_SIGMA(nf_smaller)                                          /* exact f32 only */
#undef NF_DECLARE_MLP_SIGMA
#undef NF_DECLARE_MLP_SIGMA_SPLIT
/* K5 without the colours: weights (R,S), disp (R) and acc (R) of nf_volume_render_fwd from sigma (R,S) = raw[..., 3] alone, bit for
 * bit (they depend on the density, z, |rd| and the noise only; neither the colours nor the background prior enter alpha).        */
int nf_volume_weights_fwd(const float* sigma, const float* z, const float* rd, const float* noise, int64_t n_rays, int n_samples,
                          float* disp, float* acc, float* weights, nf_stream_t stream);

/* ---- colour on live samples only (ABI 5 still: these only add) ---------------------------------------------------------------
 * nf_paper_mlp_fwd_live: nf_paper_mlp_fwd (exact f32, inference) with the colour layers run only on the samples the integrator can
 * see.  A point is live when !(sigma_raw <= 0) or it is the last sample of its ray; raw[..., 3] is nf_paper_mlp_fwd's for every
 * point, raw[..., 0:3] is nf_paper_mlp_fwd's for every live point and 0.0 for every other one, bit for bit.  nf_volume_render_fwd
 * WITHOUT a noise tensor gives the same outputs from either `raw` (alpha of a dead sample is exactly 0); with noise the ReLU
 * argument is sigma_raw + noise, and the full forward is the one to call.
 * scratch: nf_paper_mlp_fwd_live_scratch_floats(max_workgroups) floats, 16-byte aligned, contents irrelevant before and after the
 * call (each wave's ring of gathered rows); one buffer serves the launches of one stream.  max_workgroups: 0 = the persistent grid of
 * nf_paper_mlp_fwd (one workgroup per CU of the current device); > 0 caps it (a small launch then walks many blocks per wave).     */
size_t nf_paper_mlp_fwd_live_scratch_floats(int max_workgroups);
int nf_paper_mlp_fwd_live(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                          const float* z, int64_t n_rays, int n_samples, float* raw, float* scratch, size_t scratch_floats,
                          int max_workgroups, nf_stream_t stream);
/* The kernel's waves take their work in units of 32 consecutive points from a counter in device memory that the library owns: the
 * first launch on a device allocates the counters of that device (hipMalloc: make it outside a stream capture), no later one
 * allocates.  Every launch zeroes its stream's counter on that stream in front of the kernel, so launches may follow each other on
 * one stream without a synchronise and may be in flight together on several streams.
 * nf_paper_mlp_fwd_live_stats: the same launch, same `raw`, through an instantiation of the kernel that records its schedule -- an
 * instrument for tests and profiles, not a render path.  stats: int64 [stats_rows][4] on the device, 8-byte aligned, stats_rows >=
 * 4 * (workgroups of the capped grid) = scratch floats / 4416; zeroed on the stream, then row (workgroup * 4 + wave) =
 * (units of 32 points the wave took, colour runs with the final flush, rows of the final flush, wall_clock64() at exit).
 * nf_paper_mlp_fwd_live_phases: the same with rows of 4 + 6: behind those four, six sums of shader clocks over the wave's passes --
 * inputs and trunk up to the hook, hook and lone tile, ballot and append, a run's gathers up to its first MFMA, the run with its
 * stores, the stores of the rows without a colour.                                                                                 */
int nf_paper_mlp_fwd_live_phases(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                 const float* z, int64_t n_rays, int n_samples, float* raw, float* scratch, size_t scratch_floats,
                                 int max_workgroups, int64_t* stats, size_t stats_rows, nf_stream_t stream);
int nf_paper_mlp_fwd_live_stats(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                const float* z, int64_t n_rays, int n_samples, float* raw, float* scratch, size_t scratch_floats,
                                int max_workgroups, int64_t* stats, size_t stats_rows, nf_stream_t stream);

/* ---- fc_feat, too, only where it is needed (ABI 5 still: these only add) ------------------------------------------------------------
 * nf_paper_mlp_fwd_gated: nf_paper_mlp_fwd_live with the trunk ended behind layers_xyz.5.  A 256-term dot product on
 * relu(layers_xyz.5) and a rounding bound (DESIGN.md "Sigma gate") prove most samples without density dead; fc_feat and everything
 * behind it run on the others only.  Per point, against nf_paper_mlp_fwd: where !(sigma_raw <= 0), or on a ray's last sample, all four
 * channels are the same bits; elsewhere rgb is 0.0 and sigma_raw is either the same bits or some negative number (never NaN).
 * nf_volume_render_fwd WITHOUT a noise tensor gives the same outputs from either `raw`.
 * bound: nf_paper_sigma_bound_floats() floats, 16-byte aligned, written by nf_paper_sigma_bound(packed, bound, stream) from the image
 * nf_paper_pack wrote: it is valid for that image, and `cond` must be a bias table of that image.  scratch, max_workgroups, the unit
 * counters: as nf_paper_mlp_fwd_live.  nf_paper_mlp_fwd_gated_stats: stats is int64 [stats_rows][5], nf_paper_mlp_fwd_live_stats' four
 * columns (a "colour run" is a gathered run) and the rows the wave proved dead.  nf_paper_mlp_fwd_gated_phases: rows of 5 + 6, the six
 * sums of clocks of nf_paper_mlp_fwd_live_phases behind them (the lone tile is the bound tile, a run a gathered run).               */
int nf_paper_mlp_fwd_gated_phases(const float* packed, const float* bound, const float* cond, const float* ro, const float* rd,
                                  const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw, float* scratch,
                                  size_t scratch_floats, int max_workgroups, int64_t* stats, size_t stats_rows, nf_stream_t stream);
size_t nf_paper_sigma_bound_floats(void);
int nf_paper_sigma_bound(const float* packed, float* bound, nf_stream_t stream);
int nf_paper_mlp_fwd_gated(const float* packed, const float* bound, const float* cond, const float* ro, const float* rd,
                           const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw, float* scratch,
                           size_t scratch_floats, int max_workgroups, nf_stream_t stream);
int nf_paper_mlp_fwd_gated_stats(const float* packed, const float* bound, const float* cond, const float* ro, const float* rd,
                                 const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw, float* scratch,
                                 size_t scratch_floats, int max_workgroups, int64_t* stats, size_t stats_rows, nf_stream_t stream);

/* ---- isosurface of a dense grid (ABI 5 still: these only add) ------------------------------------------------------------------
 * grid: float32 [nz][ny][nx], x fastest; every axis n >= 2.  Marching tetrahedra on the Kuhn triangulation (DESIGN.md
 * "Isosurface" is the specification): a welded, consistently oriented mesh, normals from inside (v > level) to outside; vertex ids
 * in the order (k, j, i, owned edge), faces in the order (cell, tetrahedron, triangle); bit-identical from run to run (no atomics).
 * nf_isosurface_count fills `workspace` (nf_isosurface_workspace_bytes(nx, ny, nz) bytes, 8-byte aligned; 0 = a size the plan
 * does not serve: an axis below 2, or 7 * points or 12 * cells above 2^31 - 1, which bounds V and F before any launch) and writes
 * counts_dev[0] = V, counts_dev[1] = F on the device.  nf_isosurface_emit, with the same grid, sizes, level and the workspace as
 * that call left it, writes verts (V,3) f32, faces (F,3) i32 and, unless NULL, unit normals (V,3) f32 (the zero vector where the
 * interpolated gradient is zero or not finite).  n_verts / n_faces are the CAPACITIES of the output buffers in rows: no row at or
 * past them is written (the counts live on the device, so a smaller capacity truncates instead of failing); lo, hi: HOST float[3].
 * NF_EINVAL before any device call: NULL pointers (normals excepted), an unserved size, workspace_bytes too small, !(lo < hi) on an
 * axis, a negative capacity.  nf_isosurface_table: host only, the derived case table [6 tetrahedra][16 inside masks] -- six 4-bit
 * vertex codes (tet vertex lo | hi << 2: the edge lo-hi) from bit 0, the number of triangles in bits 24-25, the flip bit in bit 26
 * (the stored order has the flip applied).                                                                                      */
size_t nf_isosurface_workspace_bytes(int nx, int ny, int nz);
int nf_isosurface_count(const float* grid, int nx, int ny, int nz, float level, void* workspace, size_t workspace_bytes,
                        int64_t* counts_dev, nf_stream_t stream);
int nf_isosurface_emit(const float* grid, int nx, int ny, int nz, float level, const float* lo, const float* hi, void* workspace,
                       size_t workspace_bytes, float* verts, int64_t n_verts, int* faces, int64_t n_faces, float* normals,
                       nf_stream_t stream);
int nf_isosurface_table(uint32_t* out);

/* ---- sparse evaluation of a dense grid around one level (ABI 5 still: these only add) -------------------------------------------
 * The grid of the isosurface entry points, cut into bricks of `brick` >= 2 cells (DESIGN.md "Sparse density grid" is the
 * specification): axis a has m = ceil((n - 1) / brick) bricks, the coarse lattice is the (mx + 1)(my + 1)(mz + 1) brick corners.
 * The caller evaluates its function on the lattice, scatters the values into the grid, and then
 *   nf_sparse_grid_classify  reads the 8 corners of every brick from `grid`: a brick is a seed unless all are > level + margin or
 *                            all are < level - margin (float32 sums; NaN makes a seed), active within `dilate` bricks of a seed;
 *   nf_sparse_grid_mark      counts the points of active bricks that are no lattice points; counts_dev[0..2] = seed bricks, active
 *                            bricks, points to evaluate (int64, on the device);
 *   nf_sparse_grid_emit      writes their linear indices (ascending) and coordinates lo + i * h (multiply, then add; h = (hi - lo) /
 *                            (n - 1) in float32) to index / coords, and +inf / -inf into every grid point that is neither listed nor
 *                            on the lattice: the side (v > level or not) of the corners of the bricks it lies in.
 * `capacity` is the size of index / coords in rows: nf_sparse_grid_lattice needs at least the lattice's size; nf_sparse_grid_emit
 * writes no row at or past it.  nf_sparse_grid_scatter: grid[index[t]] = values[t] for t < count; an index outside the grid
 * writes nothing.  workspace: nf_sparse_grid_workspace_bytes(nx, ny, nz, brick) bytes, 8-byte aligned, the same buffer through
 * classify, mark and emit; 0 = a size that is not served (an axis below 2, brick below 2, or a grid past nf_isosurface's plan).
 * lo, hi: HOST float[3].  NF_EINVAL before any device call: NULL pointers, an unserved size, workspace_bytes or capacity too small,
 * !(lo < hi) on an axis, margin < 0 or NaN, dilate < 0, count < 0 or above the grid's points.  Two calls give the same bits.    */
size_t nf_sparse_grid_workspace_bytes(int nx, int ny, int nz, int brick);
int nf_sparse_grid_lattice(int nx, int ny, int nz, int brick, const float* lo, const float* hi, int* index, float* coords,
                           int64_t capacity, nf_stream_t stream);
int nf_sparse_grid_classify(const float* grid, int nx, int ny, int nz, int brick, float level, float margin, int dilate,
                            void* workspace, size_t workspace_bytes, nf_stream_t stream);
int nf_sparse_grid_mark(int nx, int ny, int nz, int brick, void* workspace, size_t workspace_bytes, int64_t* counts_dev,
                        nf_stream_t stream);
int nf_sparse_grid_emit(float* grid, int nx, int ny, int nz, int brick, const float* lo, const float* hi, void* workspace,
                        size_t workspace_bytes, int* index, float* coords, int64_t capacity, nf_stream_t stream);
int nf_sparse_grid_scatter(const float* values, const int* index, int64_t count, float* grid, int nx, int ny, int nz,
                           nf_stream_t stream);

/* ---- connected components of an indexed mesh, and the mesh of the kept ones (ABI 5 still: these only add) ------------------------
 * faces: int32 [F][3] over V vertices, 0 <= V, F < 2^31 (DESIGN.md "Mesh components" is the specification).  A face is valid iff
 * its three indices lie in [0, V); vertices are connected through valid faces (a shared vertex is enough); components are numbered
 * 0 .. C-1 by ascending smallest vertex id.  workspace: nf_mesh_components_workspace_bytes(V, F) bytes, 8-byte aligned, any content,
 * the same buffer through label, select and emit; 0 = a size that is not served (negative, or 2^31 and above).
 *   nf_mesh_components_label   vertex_label[V]; face_label[F] = the label of the face's first vertex, -1 for an invalid face;
 *                              face_counts / vertex_counts: buffers of V entries, of which the first C are written (valid faces and
 *                              vertices per component); counts_dev[0] = C (int64, on the device).
 *   nf_mesh_components_select  with those arrays and the workspace as label left it: the component with the most faces, ties to the
 *                              lower label, none if no component has a face (largest != 0, min_faces == 0), or every component with
 *                              at least min_faces >= 1 faces (largest == 0); counts_dev[1] = kept vertices, [2] = kept faces,
 *                              [3] = kept components ([0] is left alone).
 *   nf_mesh_components_emit    with the workspace as select left it: the kept vertices and the valid faces of kept components in
 *                              their original order, indices renumbered; vertex (and, unless both are NULL, normal) rows copied bit
 *                              for bit.  cap_vertices / cap_faces are the CAPACITIES of the outputs in rows: no row at or past them
 *                              is written.
 * NF_EINVAL before any device call: NULL pointers where the size is not 0, an unserved size, workspace_bytes too small, both rules
 * or neither, a negative min_faces or capacity, normals without out_normals or the reverse.  Two calls give the same bits.      */
size_t nf_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int nf_mesh_components_label(const int* faces, int64_t n_vertices, int64_t n_faces, void* workspace, size_t workspace_bytes,
                             int* vertex_label, int* face_label, int* face_counts, int* vertex_counts, int64_t* counts_dev,
                             nf_stream_t stream);
int nf_mesh_components_select(const int* vertex_label, const int* face_label, const int* face_counts, int64_t n_vertices,
                              int64_t n_faces, int largest, int64_t min_faces, void* workspace, size_t workspace_bytes,
                              int64_t* counts_dev, nf_stream_t stream);
int nf_mesh_components_emit(const float* vertices, const int* faces, const float* normals, const int* vertex_label,
                            const int* face_label, const int* face_counts, int64_t n_vertices, int64_t n_faces, void* workspace,
                            size_t workspace_bytes, float* out_vertices, int64_t cap_vertices, int* out_faces, int64_t cap_faces,
                            float* out_normals, nf_stream_t stream);

/* ---- Taubin smoothing of an indexed mesh, and the vertex normals of its faces (ABI 5 still: these only add) ------------------------
 * vertices: f32 [V][3], faces: int32 [F][3], 0 <= V < 2^31 and 0 <= 6 F < 2^31 (DESIGN.md "Mesh smoothing" is the specification).  A
 * face is valid iff its three indices lie in [0, V); a valid face (a, b, c) has the sides ab, bc, ca, a side with equal ends is
 * dropped.  workspace: nf_mesh_smooth_workspace_bytes(V, F) bytes, 8-byte aligned, any content; 0 = a size that is not served.
 *   nf_mesh_smooth_adjacency  the neighbours of every vertex as CSR: row_start[V + 1]; neighbours / multiplicity: buffers of 6 F
 *                             entries of which the first E are written -- row v holds the distinct w != v joined to v by a side,
 *                             ascending, and the number of sides joining them; boundary[V] = 1 iff v ends an edge of multiplicity
 *                             1; counts_dev[0] = E, counts_dev[1] = boundary vertices (int64, on the device).
 *   nf_mesh_smooth_run        iterations x (a pass with lam, then, unless mu == 0, a pass with mu) over a table of
 *                             nf_mesh_smooth_adjacency, all enqueued by this one call: p'[v] = p[v] + f * (mean of p over N(v) - p[v])
 *                             with the sum in ascending neighbour order and every operation rounded on its own; a vertex without
 *                             neighbours, or with pinned[v] != 0 (pinned: NULL = none), is copied.  The passes alternate between
 *                             tmp and out (V x 3 floats each; tmp may be NULL for at most one pass), the result is in out;
 *                             iterations == 0 copies.  vertices, tmp and out are three different buffers.
 *   nf_mesh_smooth_normals    normals[V][3]: the sum of (p[b] - p[a]) x (p[c] - p[a]) over the valid faces that hold the vertex, each
 *                             once, in ascending face order, divided by its length; the zero vector where that is zero or not finite.
 * NF_EINVAL before any device call: NULL pointers where the size is not 0, an unserved size, workspace_bytes too small, negative
 * iterations, lam outside (0, 1], mu outside [-1, 0], either not a number, aliased buffers.  No float atomics: two calls give the same bits. */
size_t nf_mesh_smooth_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int nf_mesh_smooth_adjacency(const int* faces, int64_t n_vertices, int64_t n_faces, void* workspace, size_t workspace_bytes,
                             int* row_start, int* neighbours, int* multiplicity, uint8_t* boundary, int64_t* counts_dev,
                             nf_stream_t stream);
int nf_mesh_smooth_run(const float* vertices, int64_t n_vertices, const int* row_start, const int* neighbours, const uint8_t* pinned,
                       int iterations, float lam, float mu, float* tmp, float* out, nf_stream_t stream);
int nf_mesh_smooth_normals(const float* vertices, const int* faces, int64_t n_vertices, int64_t n_faces, void* workspace,
                           size_t workspace_bytes, float* normals, nf_stream_t stream);

/* ---- per-vertex radiance of a mesh (ABI 5 still: these only add) ---------------------------------------------------------------------
 * DESIGN.md "Mesh colours" is the specification.  vertices, normals: f32 [V][3], 0 <= V < 2^31, the normals towards lower density;
 * 1 <= n_samples = K <= 64.
 *   nf_mesh_colour_rays       the short ray through the surface at every vertex, in the layout the forwards take (the vertices are
 *                             its origins): rd[V][3] = -normals (a sign flip); z[V][K], z[k] = float(2 k - K + 1) * (depth / float(K)),
 *                             from outside to inside; rd_view[V][3], the direction a camera would have fed the network (only its z
 *                             reaches it) -- c2w: 12 device floats, R | o, row r at c2w + r * c2w_row_stride (>= 4): t = v - o,
 *                             d = -((t0 R02 + t1 R12) + t2 R22); d > 0: t / d, else the central ray (-R02, -R12, -R22); c2w == NULL:
 *                             (0, 0, view_z).  Every operation rounded on its own, in this association.
 *   nf_mesh_colour_integrate  raw[V][K][4] (16-byte aligned), step = the samples' spacing: sigma = relu(raw[k][3]) (a NaN stays),
 *                             alpha = 1 - expf(-sigma step), w = alpha * prod_{j<k}(1 - alpha_j), opacity[V] = sum w, colour[V][3] =
 *                             sum w sigmoid(raw[k][:3]) / opacity where opacity >= min_opacity, else sigmoid(raw[K / 2][:3]); sums in
 *                             ascending k.  No background sample, nothing added to a density, no scaling by |rd|.
 * n_vertices == 0 returns 0.  NF_EINVAL before any launch: NULL pointers, K outside [1, 64], depth or step negative or not a number,
 * min_opacity not a number, a row stride below 4.  Nothing outside the named ranges is written; two calls give the same bits.      */
int nf_mesh_colour_rays(const float* vertices, const float* normals, int64_t n_vertices, const float* c2w, int64_t c2w_row_stride,
                        float view_z, int n_samples, float depth, float* rd, float* rd_view, float* z, nf_stream_t stream);
int nf_mesh_colour_integrate(const float* raw, int64_t n_vertices, int n_samples, float step, float min_opacity, float* colour,
                             float* opacity, nf_stream_t stream);

/* ---- decimation of an indexed mesh by vertex clustering, with welded faces (ABI 5 still: these only add) -----------------------------
 * DESIGN.md "Mesh decimation" is the specification.  vertices: f32 [V][3], faces: int32 [F][3], 0 <= V, F <= 2^30; origin, cell: HOST
 * float[3], the cell finite and > 0.  Per axis t = (p - o) / c in float32, i = floor(t); a vertex is clustered iff all three t are
 * finite and -2^20 <= i < 2^20, and the clustered vertices of one cell are one cluster, every other vertex a cluster of its own; the
 * representative of a cluster is its smallest vertex id.  A face with an index outside [0, V) takes no part; a valid face becomes the
 * triple of its representatives, dropped as degenerate iff two are equal; of the faces with one vertex set none is kept if as many
 * are even as odd permutations of the ascending triple, else the one of the majority orientation with the smallest face id.
 * workspace: nf_mesh_decimate_workspace_bytes(V, F) bytes, 8-byte aligned, any content; 0 = a size that is not served.
 *   nf_mesh_decimate_count    clustering, the face set, the used marks and both scans; counts_dev[8] (int64, on the device) = V', F',
 *                             degenerate faces, coincident faces (non-degenerate valid faces not kept), invalid faces, unclustered
 *                             vertices, the largest cluster, the overflow flag (a probe of a hash set visited every slot: never at
 *                             the load of at most 0.5 the plan keeps; the other counts mean nothing then).
 *   nf_mesh_decimate_emit     with the same mesh, origin and cell and the workspace as count left it: out_vertices [V'][3] = the used
 *                             representatives in ascending order -- a cluster of one member its floats bit for bit, a larger one the
 *                             mean of its members in the cell's 2^30 fixed point, order-independent; out_faces [F'][3] = the kept faces
 *                             in their order and winding, renumbered; vertex_map[V] = the new id of v's representative, -1 for a
 *                             cluster no kept face uses.  n_out_vertices / n_out_faces must be V' and F' as count found them: this
 *                             call reads those two words back (it waits for the stream) and, if they differ, writes nothing.
 * NF_EINVAL before any launch: NULL pointers where the size is not 0, an unserved size, workspace_bytes too small, a cell that is
 * NaN, infinite or <= 0, an origin that is NaN or infinite, n_out_vertices / n_out_faces other than V' / F'.  Integer atomics only:
 * two calls give the same bits.                                                                                                   */
size_t nf_mesh_decimate_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int nf_mesh_decimate_count(const float* vertices, const int* faces, int64_t n_vertices, int64_t n_faces, const float* origin,
                           const float* cell, void* workspace, size_t workspace_bytes, int64_t* counts_dev, nf_stream_t stream);
int nf_mesh_decimate_emit(const float* vertices, const int* faces, int64_t n_vertices, int64_t n_faces, const float* origin,
                          const float* cell, void* workspace, size_t workspace_bytes, float* out_vertices, int64_t n_out_vertices,
                          int* out_faces, int64_t n_out_faces, int* vertex_map, nf_stream_t stream);

/* ---- host-only self-tests (no device needed): consistency of the weight-gradient job tables -- every slab entry written
 * exactly once per slice, tile ids inside their bundle.  0 = consistent, negative = which check failed.                 */
int nf_selftest_dw_tables_f32(void);
int nf_selftest_dw_tables_lcode_f32(void);
int nf_selftest_dw_tables_smaller_f32(void);
int nf_selftest_dw_tables_bf16(void);
int nf_selftest_dw_tables_tiny(void);
int nf_selftest_dw_tables_flex(int num_layers);
/* gather tables of the four split-bf16 weight streams (host code; out == NULL: number of entries): one code per element of
 * the hi blocks, tensor id << 24 | element offset, 0xFF000000 = zero padding                                            */
long nf_paper_stream_table_bf16(uint32_t* out, size_t n_entries);
long nf_paper_stream_table_bwd_bf16(uint32_t* out, size_t n_entries);
long nf_lcode_stream_table_bf16(uint32_t* out, size_t n_entries);
long nf_lcode_stream_table_bwd_bf16(uint32_t* out, size_t n_entries);

#ifdef __cplusplus
}
#endif
#endif /* NERFACE_HIP_H */
