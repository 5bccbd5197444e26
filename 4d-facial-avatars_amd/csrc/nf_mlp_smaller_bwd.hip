// Backward of the third model family (ConditionalBlendshapePaperSmallerNeRFModel, reference nerf/models.py:266-338; autograd
// through M:313-338 as the trainer drives it): gradients w.r.t. its 22 parameter tensors and the latent code, exact f32, the three
// stages of the paper model (nf_mlp_bwd.hip) driven through one NfBwdFamily record (nf_mlp_bwd.h):
//   B1 k_smaller_mlp_bwd_chain  dZ_D2 -> dZ_D1 -> dZ_D0 -> d feat (+ d sigma * fc_alpha.weight) -> dZ_L4 -> dZ_L3 -> dZ_L2 -> dZ_L1
//                               -> dZ_L0, masks from the bit masks the training forward saved
//   B2 k_dw_gemm_lds<2>         dW = dZ^T . X over point slices (8 groups of four 128 x 128 products), bias grads as column sums
//   B3 k_grad_reduce<2>, k_smaller_grad_unpack   slabs -> the 22 reference-layout tensors: PE slot order -> columns; every folded
//                               column as (column sum of the layer's dZ) x (the constant it multiplied): expression and latent in
//                               layers_xyz.0 / .3, and in layers_dir.0 the 16 near / far columns AND the 76 expression columns;
//                               d latent = W0[:,139:171]^T db0 + W3[:,139:171]^T db3 (the latent code does not reach layers_dir.0)
#include <vector>
#include <mutex>
#include "nf_mlp_dev.h"
#include "nf_mlp_stream.h"
#include "nf_mlp_smaller_layout.h"
#include "nf_mlp_bwd.h"
#include "nf_pack.h"

// =================================================================================================
// transposed pack: block (ni, no), lane (g, i), r -> W[row = 16 ni + 4 g + r][col0 + 16 no + i]
// =================================================================================================
static void nf_smaller_table_t(std::vector<uint32_t>& t) {
    using namespace nsm;
    t.assign(PACKED_T, NF_ZERO_CODE);
    nf_fill_frag_t(t, OFFT_RGB, 1, 8, 20, 3, 128, 0);             // fc_rgb.weight (3,128)
    nf_fill_frag_t(t, OFFT_D2, 8, 8, 18, 128, 128, 0);            // layers_dir.2
    nf_fill_frag_t(t, OFFT_D1, 8, 8, 16, 128, 128, 0);            // layers_dir.1
    nf_fill_frag_t(t, OFFT_D0, 8, 16, 14, 128, 356, 0);           // layers_dir.0[:, :256]
    nf_fill_frag_t(t, OFFT_D0 + 8 * 16 * FRAG, 1, 16, 12, 1, 256, 0);   // chunk 8: slot 0 = fc_alpha.weight (1,256)
    nf_fill_frag_t(t, OFFT_FEAT, 16, 16, 10, 256, 256, 0);        // fc_feat
    nf_fill_frag_t(t, OFFT_L4, 16, 16, 8, 256, 256, 0);
    nf_fill_frag_t(t, OFFT_L3, 16, 16, 6, 256, 427, 171);         // layers_xyz.3[:, 171:427]
    nf_fill_frag_t(t, OFFT_L2, 16, 16, 4, 256, 256, 0);
    nf_fill_frag_t(t, OFFT_L1, 16, 16, 2, 256, 256, 0);
}

static NfPackTable g_smaller_table_t;

extern "C" size_t nf_smaller_packed_bwd_floats(void) { return (size_t)nsm::PACKED_T; }

extern "C" int nf_smaller_pack_bwd(const float* const* params, float* packed_t, nf_stream_t stream) {
    return nf_pack_f32<nsm::NPARAMS, 9>(g_smaller_table_t, nf_smaller_table_t, params, packed_t, (int)nsm::PACKED_T, stream);
}

// =================================================================================================
// B1: backward chain
// =================================================================================================
// Layer-streamed like the paper model's chain (nf_mlp_bwd.hip: k_paper_mlp_bwd_chain_masks; nf_mlp_stream.h: nf_seg_lds, nf_tail_dz):
// C = 0 as the C operand of a layer's first MFMAs, the slab copied to `dz` from inside the K loops, the masked layer boundary under the
// last chunk, a layer's two mask words fetched when its loop starts.  ReLU layers: layers_xyz.0..4 -> 0..4, layers_dir.0..2 -> 5..7.
template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_smaller_mlp_bwd_chain(const float* __restrict__ packed_t, const float* __restrict__ saved, const float* __restrict__ d_raw,
                        int64_t n_points, float* __restrict__ dz) {
    using namespace nsm;
    static_assert(NT == 2, "the copy schedule below is written for 32-point slabs");
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int64_t p0 = ((int64_t)blockIdx.x * NF_MLP_WAVES + wave) * (16 * NT);
    if (p0 >= n_points) return;
    f32x4* act4 = lds + wave * (16 * NT * 64);
    const int64_t n = n_points;
    const NfW Wi = nf_w_image(packed_t, PACKED_T);
    auto sec = [&](int zs, int width) { return nf_slab_copy(dz, zs, width, p0, n); };
    auto masks = [&](int l, uint2 (&m)[NT]) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
            m[t] = p0 + 16 * t < n ? *nf_mask_ptr<S_MASK>(const_cast<float*>(saved), n, l, (p0 >> 4) + t, lane) : make_uint2(0u, 0u);
    };
    f32x4 frag_rgb[NT][1], frag_sig[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int64_t p = p0 + 16 * t + c;
        f32x4 d = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (p < n && g == 0) d = reinterpret_cast<const f32x4*>(d_raw)[p];
        frag_rgb[t][0] = (f32x4){d.x, d.y, d.z, 0.f};
        frag_sig[t] = (f32x4){d.w, 0.f, 0.f, 0.f};
    }
    f32x4 acc[NT][16];
    NfStream<NT> st;
    f32x4 bj[NT];
    uint64_t unused64[NT];
    uint2 m[NT];
#pragma unroll
    for (int no = 0; no < 16; ++no) st.bias[no] = (f32x4){0.f, 0.f, 0.f, 0.f};      // C = 0: the C operand of every layer's first MFMAs
    // d(layers_dir.2 out) = d rgb . fc_rgb.weight, masked by layers_dir.2's ReLU: one register chunk
    masks(7, m);
    nf_zero_acc<NT, 8>(acc);
    nf_mma_from_regs<NT, 8, 1>(acc, reinterpret_cast<const f32x4*>(packed_t) + OFFT_RGB / 4, frag_rgb, lane);
    nf_apply_mask<NT, 8>(acc, m);
    nf_store_act<NT, 8, false>(acc, act4, lane);
    nf_load_w16<8>(st.wa, Wi, OFFT_D2 / 4, lane);
    nf_read_b<NT>(st.b0, act4, lane, 0);
    // one layer from the slab: the slab = dZ section ZSEC_ (W4_ float4 per row) is copied out and consumed; the output is masked by
    // ReLU layer MASKL_ under the last chunk and becomes the next slab
#define NF_SM_CHAIN_LAYER(OFF_, NO_, NCH_, W4_, ZSEC_, MASKL_, OFF_NEXT_, NO_NEXT_)                                    \
    do {                                                                                                             \
        NfCopyH<W4_, 4, false> cs{act4, sec(ZSEC_, 4 * (W4_)), lane, (NCH_) / 2, {}};                                  \
        cs.prime();                                                                                                  \
        masks(MASKL_, m);                                                                                            \
        nf_seg_lds<NT, NO_, true, false, false>(acc, st, Wi, OFF_, NCH_, act4, lane, cs, unused64);                  \
        nf_pending_b<NT, false>(bj, st);                                                                             \
        nf_tail_dz<NT, NO_, NO_NEXT_, true>(acc, st.wb, bj, st, Wi, OFF_NEXT_, act4, lane, m);                       \
    } while (0)
    NF_SM_CHAIN_LAYER(OFFT_D2 / 4, 8, 8, 32, Z_D2, 6, OFFT_D1 / 4, 8);
    NF_SM_CHAIN_LAYER(OFFT_D1 / 4, 8, 8, 32, Z_D1, 5, OFFT_D0 / 4, 16);
    // d feat = dZ_D0 . layers_dir.0.weight[:, :256] + d sigma * fc_alpha.weight   (no activation on feat): 8 slab chunks + one register chunk
    {
        f32x4 wd[16];
        nf_load_w16<16>(wd, Wi, OFFT_D0 / 4 + 8 * 16 * 64, lane);          // the d-sigma chunk's weights, a layer ahead
        NfCopyH<32, 4, false> cs{act4, sec(Z_D0, 128), lane, 4, {}};
        cs.prime();
        nf_seg_lds<NT, 16, true, false, false>(acc, st, Wi, OFFT_D0 / 4, 8, act4, lane, cs, unused64);
        nf_pending_b<NT, false>(bj, st);
        nf_chunk<NT, 16, false>(acc, st.wb, bj, st.bias);
        nf_tail_dz<NT, 16, 16, false>(acc, wd, frag_sig, st, Wi, OFFT_FEAT / 4, act4, lane, m);
    }
    NF_SM_CHAIN_LAYER(OFFT_FEAT / 4, 16, 16, 64, Z_FEAT, 4, OFFT_L4 / 4, 16);
    NF_SM_CHAIN_LAYER(OFFT_L4 / 4, 16, 16, 64, Z_L4, 3, OFFT_L3 / 4, 16);
    NF_SM_CHAIN_LAYER(OFFT_L3 / 4, 16, 16, 64, Z_L3, 2, OFFT_L2 / 4, 16);       // hidden columns of the skip layer only
    NF_SM_CHAIN_LAYER(OFFT_L2 / 4, 16, 16, 64, Z_L2, 1, OFFT_L1 / 4, 16);
    NF_SM_CHAIN_LAYER(OFFT_L1 / 4, 16, 16, 64, Z_L1, 0, 0, 0);
#undef NF_SM_CHAIN_LAYER
    {   // the last section has no K loop behind it
        const NfSlabCopy cp = sec(Z_L0, 256);
#pragma unroll 4
        for (int k = 0; k < 16 * NT; ++k) nf_copy_rows<64>(act4, cp, k, lane);
    }
}

// =================================================================================================
// B2 job table: the 32 products (128 x 128 each) as groups of four that share operand panels (k_dw_gemm_lds, nf_mlp_dw.h)
// =================================================================================================
#define NF_SM_DW_GROUPS 8

static void nf_smaller_build_dw_groups(NfDwGroup* gr) {
    using namespace nsm;
    int n = 0;
    const NfDwPanel off{-1, 0, 0, 0, 0};
    auto fresh = [&]() -> NfDwGroup& {
        NfDwGroup& g = gr[n++];
        for (auto& p : g.panel) p = off;
        g.share = 2;
        g.n_slices = g.pts_per_slice = 0;
        return g;
    };
    auto job = [](const NfDwGroup& g, int a, int b, int out_off, int ldo, int cs) {
        return NfDwWaveJob{a, b, g.panel[a].valid, g.panel[b].valid, out_off, ldo, cs};
    };
    // a 256 x 256 layer: panels {dZ lo, dZ hi, X lo, X hi}, waves = the 2 x 2 blocks of the product
    auto layer256 = [&](int zsec, int bsec, int gout, int cs) {
        NfDwGroup& g = fresh();
        for (int h = 0; h < 2; ++h) {
            g.panel[h] = NfDwPanel{0, zsec, 256, 128 * h, 128};
            g.panel[2 + h] = NfDwPanel{2, bsec, 256, 128 * h, 128};
        }
        for (int nb = 0; nb < 2; ++nb)
            for (int kb = 0; kb < 2; ++kb)
                g.wave[2 * nb + kb] = job(g, nb, 2 + kb, gout + 128 * nb * 256 + 128 * kb, 256, (kb == 0 && cs >= 0) ? cs + 128 * nb : -1);
    };
    layer256(Z_L1, S_H0, G_L1, CS_L0 + 256);
    layer256(Z_L2, S_H1, G_L2, CS_L0 + 512);
    layer256(Z_L3, S_H2, G_L3B, -1);
    layer256(Z_L4, S_H3, G_L4, CS_L0 + 1024);
    layer256(Z_FEAT, S_H4, G_FEAT, CS_L0 + 1280);
    {   // the four products against the positional encoding: (dZ_L0 | dZ_L3) x PE
        NfDwGroup& g = fresh();
        for (int h = 0; h < 2; ++h) {
            g.panel[h] = NfDwPanel{0, Z_L0, 256, 128 * h, 128};
            g.panel[2 + h] = NfDwPanel{0, Z_L3, 256, 128 * h, 128};
        }
        g.panel[4] = NfDwPanel{2, S_PE, 64, 0, 64};
        g.share = 1;                                                 // second halves idle: half the MFMAs per point
        for (int nb = 0; nb < 2; ++nb) {
            g.wave[nb] = job(g, nb, 4, G_L0 + 128 * nb * 64, 64, CS_L0 + 128 * nb);
            g.wave[2 + nb] = job(g, 2 + nb, 4, G_L3A + 128 * nb * 64, 64, CS_L0 + 768 + 128 * nb);
        }
    }
    {   // dZ_D0 x (feat | dir slots), dZ_D1 x d0; the column sums of dZ_D0 also carry the folded expression / near / far columns
        NfDwGroup& g = fresh();
        g.panel[0] = NfDwPanel{0, Z_D0, 128, 0, 128};
        g.panel[1] = NfDwPanel{2, S_FEAT, 256, 0, 128};
        g.panel[2] = NfDwPanel{2, S_FEAT, 256, 128, 128};
        g.panel[3] = NfDwPanel{2, S_DIRF, 16, 0, 16};
        g.panel[4] = NfDwPanel{0, Z_D1, 128, 0, 128};
        g.panel[5] = NfDwPanel{2, S_D0, 128, 0, 128};
        g.wave[0] = job(g, 0, 1, G_D0A, 256, CS_D0);
        g.wave[1] = job(g, 0, 2, G_D0A + 128, 256, -1);
        g.wave[2] = job(g, 0, 3, G_D0B, 16, -1);
        g.wave[3] = job(g, 4, 5, G_D1, 128, CS_D0 + 128);
    }
    {   // dZ_D2 x d1, d_raw x (d2 | feat): rows 0..2 = fc_rgb.weight, row 3 (d sigma) = fc_alpha.weight, cs = the 4 output-bias gradients
        NfDwGroup& g = fresh();
        g.panel[0] = NfDwPanel{0, Z_D2, 128, 0, 128};
        g.panel[1] = NfDwPanel{2, S_D1, 128, 0, 128};
        g.panel[2] = NfDwPanel{1, 0, 4, 0, 4};
        g.panel[3] = NfDwPanel{2, S_D2, 128, 0, 128};
        g.panel[4] = NfDwPanel{2, S_FEAT, 256, 0, 128};
        g.panel[5] = NfDwPanel{2, S_FEAT, 256, 128, 128};
        g.wave[0] = job(g, 0, 1, G_D2, 128, CS_D0 + 256);
        g.wave[1] = job(g, 2, 3, G_RGB, 128, CS_RGB);
        g.wave[2] = job(g, 2, 4, G_ALPHA, 256, -1);
        g.wave[3] = job(g, 2, 5, G_ALPHA + 128, 256, -1);
    }
    // n == NF_SM_DW_GROUPS by construction
}

// =================================================================================================
// B3, second half: scatter to the reference parameter layout (state_dict order)
// =================================================================================================
// off[t]: first flat element of tensor t; blk[t]: first workgroup of tensor t (a workgroup handles 256 elements of ONE tensor, so
// the tensor id -- and with it the switch below -- is uniform); tensor 22 = d latent
struct NfSmallerGradOffsets { int off[nsm::NPARAMS + 2]; int blk[nsm::NPARAMS + 2]; };

__global__ void __launch_bounds__(256) k_smaller_grad_unpack(const float* __restrict__ sum, const float* __restrict__ packed,
                                                             const float* __restrict__ cond, NfSmallerGradOffsets offs,
                                                             float* __restrict__ grads) {
    using namespace nsm;
    const float* cvec = cond + B_CVEC;
    const float* dvec = cond + B_DVEC;
    int t = 0;
    while ((int)blockIdx.x >= offs.blk[t + 1]) ++t;                 // uniform
    const int local = ((int)blockIdx.x - offs.blk[t]) * 256 + (int)threadIdx.x;
    if (t == NPARAMS) {
        // d latent_j = sum_n W0[n][139+j] db0[n] + W3[n][139+j] db3[n]: thread (q, j) sums n = 32 q .. 32 q + 31, the eight partial sums
        // of a j are added in a fixed order (deterministic)
        __shared__ float part[8][32];
        const int j = (int)threadIdx.x & 31, q = (int)threadIdx.x >> 5;
        const float* w0 = packed + OFF_WC0 + 76 + j;
        const float* w3 = packed + OFF_WC3 + 76 + j;
        float v = 0.f;
#pragma unroll 8
        for (int n = 32 * q; n < 32 * q + 32; ++n) v += w0[n * NCOND] * sum[CS_L0 + n] + w3[n * NCOND] * sum[CS_L0 + 768 + n];
        part[q][j] = v;
        __syncthreads();
        if (threadIdx.x < 32) {
            float r = part[0][j];
#pragma unroll
            for (int k = 1; k < 8; ++k) r += part[k][j];
            grads[offs.off[t] + j] = r;
        }
        return;
    }
    if (local >= offs.off[t + 1] - offs.off[t]) return;
    float v = 0.f;
    switch (t) {
        case 0: {  // layers_xyz.0.weight [256][171]
            const int n = local / 171, col = local - 171 * n;
            v = col < 63 ? sum[G_L0 + n * 64 + nfl::pe_col_to_slot(col)] : sum[CS_L0 + n] * cvec[col - 63];
        } break;
        case 1: v = sum[CS_L0 + local]; break;
        case 2: v = sum[G_L1 + local]; break;
        case 3: v = sum[CS_L0 + 256 + local]; break;
        case 4: v = sum[G_L2 + local]; break;
        case 5: v = sum[CS_L0 + 512 + local]; break;
        case 6: {  // layers_xyz.3.weight [256][427] = [pe 63 | cond 108 | hidden 256]
            const int n = local / 427, col = local - 427 * n;
            v = col < 63 ? sum[G_L3A + n * 64 + nfl::pe_col_to_slot(col)]
                         : (col < 171 ? sum[CS_L0 + 768 + n] * cvec[col - 63] : sum[G_L3B + n * 256 + (col - 171)]);
        } break;
        case 7: v = sum[CS_L0 + 768 + local]; break;
        case 8: v = sum[G_L4 + local]; break;
        case 9: v = sum[CS_L0 + 1024 + local]; break;
        case 10: v = sum[G_FEAT + local]; break;
        case 11: v = sum[CS_L0 + 1280 + local]; break;
        case 12: v = sum[G_ALPHA + 3 * 256 + local]; break;   // fc_alpha.weight [1][256] = row 3 (d sigma) of d_raw^T feat
        case 13: v = sum[CS_RGB + 3]; break;                  // fc_alpha.bias
        case 14: {  // layers_dir.0.weight [128][356] = [feat 256 | PE4(rd_z, near, far) 24 | expr/3 76]
            const int n = local / 356, col = local - 356 * n;
            if (col < 256) v = sum[G_D0A + n * 256 + col];
            else if (col < 280) {
                const int q = col - 256, f = q / 6, rem = q - 6 * f, sc = rem / 3, comp = rem - 3 * sc;
                v = comp == 0 ? sum[G_D0B + n * 16 + 4 * f + sc] : sum[CS_D0 + n] * dvec[4 * f + 2 * sc + (comp - 1)];
            } else v = sum[CS_D0 + n] * cvec[col - 280];
        } break;
        case 15: v = sum[CS_D0 + local]; break;
        case 16: v = sum[G_D1 + local]; break;
        case 17: v = sum[CS_D0 + 128 + local]; break;
        case 18: v = sum[G_D2 + local]; break;
        case 19: v = sum[CS_D0 + 256 + local]; break;
        case 20: v = sum[G_RGB + local]; break;               // fc_rgb.weight [3][128]
        case 21: v = sum[CS_RGB + local]; break;
    }
    grads[offs.off[t] + local] = v;
}

static const int NF_SM_PARAM_NUMEL[nsm::NPARAMS] = {
    256 * 171, 256, 65536, 256, 65536, 256, 256 * 427, 256, 65536, 256,   // layers_xyz.0..4
    65536, 256, 256, 1,                                                  // fc_feat, fc_alpha
    128 * 356, 128, 16384, 128, 16384, 128,                              // layers_dir.0..2
    384, 3};                                                             // fc_rgb

extern "C" size_t nf_smaller_grad_floats(void) { return (size_t)nsm::GRAD_FLOATS; }

static int nf_smaller_chain_f32(const void* packed_t, const float* saved, const float* d_raw, int64_t n_points, float* dz, float*,
                                nf_stream_t stream) {
    const int64_t per_block = (int64_t)NF_MLP_WAVES * 16 * NF_MLP_NT;
    hipLaunchKernelGGL((k_smaller_mlp_bwd_chain<NF_MLP_NT>), dim3((unsigned)((n_points + per_block - 1) / per_block)),
                       dim3(64 * NF_MLP_WAVES), 0, nf_s(stream), (const float*)packed_t, saved, d_raw, n_points, dz);
    return 0;
}

// this family has no split arithmetic: the record's split slots answer NF_EINVAL
static int nf_smaller_chain_none(const void*, const float*, const float*, int64_t, float*, float*, nf_stream_t) { return NF_EINVAL; }

static void nf_smaller_dw_f32(const NfDwGroupSet& gset, const float* dz, const float* d_raw, const float* saved, int64_t n_points,
                              float* slabs, hipStream_t s) {
    hipLaunchKernelGGL((k_dw_gemm_lds<2>), dim3(gset.first_block[NF_SM_DW_GROUPS]), dim3(64 * NF_DW_WAVES), 0, s, gset, (int)nsm::SLAB_FLOATS,
                       dz, d_raw, saved, n_points, slabs);
}

static void nf_smaller_reduce_unpack(const float* slabs, int ns, const NfReduceAlt& alt, float* sum, const float* packed, const float* cond,
                                     float* grads, hipStream_t s) {
    hipLaunchKernelGGL((k_grad_reduce<2>), dim3(512), dim3(256), 0, s, slabs, ns, (int)nsm::SLAB_FLOATS, sum, alt);
    NfSmallerGradOffsets offs;
    offs.off[0] = offs.blk[0] = 0;
    for (int i = 0; i <= nsm::NPARAMS; ++i) {                         // 22 tensors, then the 32 latent-code gradients
        const int numel = i < nsm::NPARAMS ? NF_SM_PARAM_NUMEL[i] : 32;
        offs.off[i + 1] = offs.off[i] + numel;
        offs.blk[i + 1] = offs.blk[i] + (numel + 255) / 256;
    }
    hipLaunchKernelGGL(k_smaller_grad_unpack, dim3(offs.blk[nsm::NPARAMS + 1]), dim3(256), 0, s, sum, packed, cond, offs, grads);
}

static const NfBwdFamily nf_smaller_bwd = {2, nsm::DZ_PER_POINT, nsm::SLAB_FLOATS, NF_SM_DW_GROUPS, nf_smaller_build_dw_groups,
                                           {nf_smaller_chain_f32, nf_smaller_chain_none, nf_smaller_chain_none},
                                           nf_smaller_dw_f32, nf_smaller_reduce_unpack};

extern "C" size_t nf_smaller_bwd_workspace_floats(int64_t n_points) { return nf_bwd_workspace_floats(nf_smaller_bwd, n_points); }

// grads: nf_smaller_grad_floats() floats = the 22 tensors in state_dict order, flattened, then d latent (32)
extern "C" int nf_smaller_mlp_bwd(const float* packed, const float* packed_t, const float* cond, const float* saved,
                                  const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                  float* grads, nf_stream_t stream) {
    return nf_bwd_run(nf_smaller_bwd, 0, packed, packed_t, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads, stream);
}

// Measurement hook (tools/time_smaller.py), as nf_paper_mlp_bwd_stage_ms for the exact-f32 backward: stage_ms[3] (host) =
// {dX chain, weight-gradient GEMMs, slab reduction + unpack} in milliseconds; synchronises the stream.
extern "C" int nf_smaller_mlp_bwd_stage_ms(const float* packed, const float* packed_t, const float* cond, const float* saved,
                                           const float* d_raw, int64_t n_rays, int n_samples, float* workspace, size_t workspace_floats,
                                           float* grads, float* stage_ms, nf_stream_t stream) {
    if (!stage_ms) return NF_EINVAL;
    return nf_bwd_run(nf_smaller_bwd, 0, packed, packed_t, cond, saved, d_raw, n_rays, n_samples, workspace, workspace_floats, grads,
                      stream, stage_ms);
}

// host-only self-test of this family's exact-f32 group table (tests/test_smaller_host.py)
extern "C" int nf_selftest_dw_tables_smaller_f32(void) {
    const long smaller = 2L * 256 * 64 + 5L * 65536 + 128L * 272 + 2L * 128 * 128 + 4L * 128 + 4L * 256 + 6 * 256 + 3 * 128 + 4;
    NfDwGroup groups[NF_SM_DW_GROUPS];
    nf_smaller_build_dw_groups(groups);
    int rc = nf_check_dw_groups(groups, NF_SM_DW_GROUPS, nsm::SLAB_FLOATS, smaller);
    if (rc) return rc;
    // the plan at the training sizes: one workgroup per CU at most, and the reduction can describe the short groups
    for (int64_t n : {(int64_t)131072, (int64_t)262144, (int64_t)259969, (int64_t)512}) {
        int first[NF_DW_MAX_GROUPS + 1];
        const int most = nf_dw_plan_groups(groups, NF_SM_DW_GROUPS, n, first);
        NfReduceAlt alt;
        if (first[NF_SM_DW_GROUPS] > 256 || most < 1 || !nf_dw_reduce_alt(groups, NF_SM_DW_GROUPS, most, &alt)) return -200;
        for (int i = 0; i < NF_SM_DW_GROUPS; ++i)
            if ((int64_t)groups[i].n_slices * groups[i].pts_per_slice < n || (groups[i].pts_per_slice & 15)) return -201;
    }
    return 0;
}
