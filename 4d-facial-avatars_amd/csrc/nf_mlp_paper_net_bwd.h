// Backward half of the exact-f32 paper-shaped network (nf_mlp_paper_net.h: NfPaperNet, NfSmallerNet), written once for both
// families: transposed gather table, the dX chain of one wave, the weight-gradient job table, the scatter into the reference-layout
// tensors and the launchers an NfBwdFamily record (nf_mlp_bwd.h) points to.  The __global__ kernels keep their names in
// nf_mlp_bwd.hip / nf_mlp_smaller_bwd.hip and wrap these.
#pragma once
#include "nf_mlp_paper_net.h"
#include "nf_mlp_bwd.h"

// =================================================================================================
// transposed pack: block (ni, no), lane (g, i), r -> W[row = 16 ni + 4 g + r][col0 + 16 no + i]   (nf_pack.h: nf_fill_frag_t)
// =================================================================================================
template <class Net>
static void nf_paper_net_table_t(std::vector<uint32_t>& t) {
    auto id = [](int role) { return nf_net_id<Net>(role); };
    t.assign(Net::PACKED_T, NF_ZERO_CODE);
    nf_fill_frag_t(t, Net::OFFT_RGB, 1, 8, id(NF_R_RGB_W), 3, 128, 0);                        // fc_rgb.weight (3,128)
    nf_fill_frag_t(t, Net::OFFT_D2, 8, 8, id(NF_R_DIR2_W), 128, 128, 0);                      // layers_dir.2
    nf_fill_frag_t(t, Net::OFFT_D1, 8, 8, id(NF_R_DIR1_W), 128, 128, 0);                      // layers_dir.1
    nf_fill_frag_t(t, Net::OFFT_D0, 8, 16, id(NF_R_DIR0_W), 128, Net::D0_COLS, 0);            // layers_dir.0[:, :256]
    nf_fill_frag_t(t, Net::OFFT_D0 + 8 * 16 * Net::FRAG, 1, 16, id(NF_R_ALPHA_W), 1, 256, 0); // chunk 8: slot 0 = fc_alpha.weight (1,256)
    nf_fill_frag_t(t, Net::OFFT_FEAT, 16, 16, id(NF_R_FEAT_W), 256, 256, 0);                  // fc_feat
    if constexpr (Net::HAS_L5) nf_fill_frag_t(t, Net::OFFT_L5, 16, 16, NF_R_L5_W, 256, 256, 0);
    nf_fill_frag_t(t, Net::OFFT_L4, 16, 16, 8, 256, 256, 0);
    nf_fill_frag_t(t, Net::OFFT_L3, 16, 16, NF_R_XYZ3_W, 256, 427, 171);                      // layers_xyz.3[:, 171:427]
    nf_fill_frag_t(t, Net::OFFT_L2, 16, 16, 4, 256, 256, 0);
    nf_fill_frag_t(t, Net::OFFT_L1, 16, 16, 2, 256, 256, 0);
}

// =================================================================================================
// B1: backward chain of one wave
// =================================================================================================
// dZ_D2 -> dZ_D1 -> dZ_D0 -> d feat (+ d sigma * fc_alpha.weight) -> (dZ_L5 ->) dZ_L4 -> ... -> dZ_L0: the layer list on the shared
// chain text (nf_mlp_net_common.h: NF_NET_CHAIN_*).
// Against the earlier block epilogue: 1.87 -> 1.78-1.80 ms per 262144 points, bit-identical (profiles/r04_experiments.md section 8).
template <class Net, int NT>
__device__ __forceinline__ void nf_paper_net_bwd_chain(f32x4* lds, const float* __restrict__ packed_t, const float* __restrict__ saved,
                                                       const float* __restrict__ d_raw, int64_t n_points, float* __restrict__ dz) {
    constexpr int NX = nf_net_n_xyz<Net>;             // ReLU layers: layers_xyz.l -> l, layers_dir.d -> NX + d
    // d(layers_dir.2 out) = d rgb . fc_rgb.weight, masked by layers_dir.2's ReLU
    NF_NET_CHAIN_BEGIN(NX + 2, Net::OFFT_D2 / 4, 8);
    NF_NET_CHAIN_LAYER(Net::OFFT_D2 / 4, 8, 8, 32, Net::Z_D2, NX + 1, Net::OFFT_D1 / 4, 8);
    NF_NET_CHAIN_LAYER(Net::OFFT_D1 / 4, 8, 8, 32, Net::Z_D1, NX, Net::OFFT_D0 / 4, 16);
    // d feat = dZ_D0 . layers_dir.0.weight[:, :256] + d sigma * fc_alpha.weight   (no activation on feat): 8 slab chunks + one register chunk
    {
        f32x4 wd[16];
        nf_load_w16<16>(wd, Wi, Net::OFFT_D0 / 4 + 8 * 16 * 64, lane);     // the d-sigma chunk's weights, a layer ahead
        NfCopyH<32, 4, false> cs{act4, sec(Net::Z_D0, 128), lane, 4, {}};
        cs.prime();
        nf_seg_lds<NT, 16, true, false, false>(acc, st, Wi, Net::OFFT_D0 / 4, 8, act4, lane, cs, unused64);
        nf_pending_b<NT, false>(bj, st);
        nf_chunk<NT, 16, false>(acc, st.wb, bj, st.bias);
        nf_tail_dz<NT, 16, 16, false>(acc, wd, frag_sig, st, Wi, Net::OFFT_FEAT / 4, act4, lane, m);
    }
    if constexpr (Net::HAS_L5) {
        NF_NET_CHAIN_LAYER(Net::OFFT_FEAT / 4, 16, 16, 64, Net::Z_FEAT, 5, Net::OFFT_L5 / 4, 16);
        NF_NET_CHAIN_LAYER(Net::OFFT_L5 / 4, 16, 16, 64, Net::Z_L5, 4, Net::OFFT_L4 / 4, 16);
    } else {
        NF_NET_CHAIN_LAYER(Net::OFFT_FEAT / 4, 16, 16, 64, Net::Z_FEAT, 4, Net::OFFT_L4 / 4, 16);
    }
    NF_NET_CHAIN_LAYER(Net::OFFT_L4 / 4, 16, 16, 64, Net::Z_L4, 3, Net::OFFT_L3 / 4, 16);
    NF_NET_CHAIN_LAYER(Net::OFFT_L3 / 4, 16, 16, 64, Net::Z_L3, 2, Net::OFFT_L2 / 4, 16);       // hidden columns of the skip layer only
    NF_NET_CHAIN_LAYER(Net::OFFT_L2 / 4, 16, 16, 64, Net::Z_L2, 1, Net::OFFT_L1 / 4, 16);
    NF_NET_CHAIN_LAYER(Net::OFFT_L1 / 4, 16, 16, 64, Net::Z_L1, 0, 0, 0);
    NF_NET_CHAIN_END(Net::Z_L0);
}

// `chain` = the family's k_*_mlp_bwd_chain*<NF_MLP_NT>
template <class Chain>
static inline int nf_paper_net_chain_launch(Chain chain, const void* packed_t, const float* saved, const float* d_raw, int64_t n_points,
                                            float* dz, nf_stream_t stream) {
    const int64_t per_block = (int64_t)NF_MLP_WAVES * 16 * NF_MLP_NT;
    hipLaunchKernelGGL(chain, dim3((unsigned)((n_points + per_block - 1) / per_block)), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream),
                       (const float*)packed_t, saved, d_raw, n_points, dz);
    return 0;
}

// =================================================================================================
// B2: weight-gradient GEMMs (generic kernel in nf_mlp_dw.h); the job table
// =================================================================================================
// The 128 x 128 products as groups of four that share operand panels (k_dw_gemm_lds): one group per 256 x 256 layer, then three
template <class Net> constexpr int nf_net_dw_groups = nf_net_n_xyz<Net> + 3;

template <class Net>
static void nf_paper_net_build_dw_groups(NfDwGroup* gr) {
    constexpr int NX = nf_net_n_xyz<Net>;
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
    // the column sums (bias gradients) of the 256-wide layers: layers_xyz.l at CS_L0 + 256 l, fc_feat behind them
    layer256(Net::Z_L1, Net::S_H0, Net::G_L1, Net::CS_L0 + 256);
    layer256(Net::Z_L2, Net::S_H1, Net::G_L2, Net::CS_L0 + 512);
    layer256(Net::Z_L3, Net::S_H2, Net::G_L3B, -1);
    layer256(Net::Z_L4, Net::S_H3, Net::G_L4, Net::CS_L0 + 1024);
    if constexpr (Net::HAS_L5) {
        layer256(Net::Z_L5, Net::S_H4, Net::G_L5, Net::CS_L0 + 1280);
        layer256(Net::Z_FEAT, Net::S_H5, Net::G_FEAT, Net::CS_L0 + 256 * NX);
    } else {
        layer256(Net::Z_FEAT, Net::S_H4, Net::G_FEAT, Net::CS_L0 + 256 * NX);
    }
    {   // the four products against the positional encoding: (dZ_L0 | dZ_L3) x PE
        NfDwGroup& g = fresh();
        for (int h = 0; h < 2; ++h) {
            g.panel[h] = NfDwPanel{0, Net::Z_L0, 256, 128 * h, 128};
            g.panel[2 + h] = NfDwPanel{0, Net::Z_L3, 256, 128 * h, 128};
        }
        g.panel[4] = NfDwPanel{2, Net::S_PE, 64, 0, 64};
        g.share = 1;                                                 // second halves idle: half the MFMAs per point
        for (int nb = 0; nb < 2; ++nb) {
            g.wave[nb] = job(g, nb, 4, Net::G_L0 + 128 * nb * 64, 64, Net::CS_L0 + 128 * nb);
            g.wave[2 + nb] = job(g, 2 + nb, 4, Net::G_L3A + 128 * nb * 64, 64, Net::CS_L0 + 768 + 128 * nb);
        }
    }
    {   // dZ_D0 x (feat | dir slots), dZ_D1 x d0; the column sums of dZ_D0 also carry the folded near / far (and expression) columns
        NfDwGroup& g = fresh();
        g.panel[0] = NfDwPanel{0, Net::Z_D0, 128, 0, 128};
        g.panel[1] = NfDwPanel{2, Net::S_FEAT, 256, 0, 128};
        g.panel[2] = NfDwPanel{2, Net::S_FEAT, 256, 128, 128};
        g.panel[3] = NfDwPanel{2, Net::S_DIRF, 16, 0, 16};
        g.panel[4] = NfDwPanel{0, Net::Z_D1, 128, 0, 128};
        g.panel[5] = NfDwPanel{2, Net::S_D0, 128, 0, 128};
        g.wave[0] = job(g, 0, 1, Net::G_D0A, 256, Net::CS_D0);
        g.wave[1] = job(g, 0, 2, Net::G_D0A + 128, 256, -1);
        g.wave[2] = job(g, 0, 3, Net::G_D0B, 16, -1);
        g.wave[3] = job(g, 4, 5, Net::G_D1, 128, Net::CS_D0 + 128);
    }
    {   // dZ_D2 x d1, d_raw x (d2 | feat): rows 0..2 = fc_rgb.weight, row 3 (d sigma) = fc_alpha.weight, cs = the 4 output-bias gradients
        NfDwGroup& g = fresh();
        g.panel[0] = NfDwPanel{0, Net::Z_D2, 128, 0, 128};
        g.panel[1] = NfDwPanel{2, Net::S_D1, 128, 0, 128};
        g.panel[2] = NfDwPanel{1, 0, 4, 0, 4};
        g.panel[3] = NfDwPanel{2, Net::S_D2, 128, 0, 128};
        g.panel[4] = NfDwPanel{2, Net::S_FEAT, 256, 0, 128};
        g.panel[5] = NfDwPanel{2, Net::S_FEAT, 256, 128, 128};
        g.wave[0] = job(g, 0, 1, Net::G_D2, 128, Net::CS_D0 + 256);
        g.wave[1] = job(g, 2, 3, Net::G_RGB, 128, Net::CS_RGB);
        g.wave[2] = job(g, 2, 4, Net::G_ALPHA, 256, -1);
        g.wave[3] = job(g, 2, 5, Net::G_ALPHA + 128, 256, -1);
    }
    // n == nf_net_dw_groups<Net> by construction
}

template <class Net>
static void nf_paper_net_dw_f32(const NfDwGroupSet& gset, const float* dz, const float* d_raw, const float* saved, int64_t n_points,
                                float* slabs, hipStream_t s) {
    hipLaunchKernelGGL((k_dw_gemm_lds<Net::MODEL>), dim3(gset.first_block[nf_net_dw_groups<Net>]), dim3(64 * NF_DW_WAVES), 0, s, gset,
                       (int)Net::SLAB_FLOATS, dz, d_raw, saved, n_points, slabs);
}

// host-only self-test of a family's exact-f32 group table (tests/test_host.py, tests/test_smaller_host.py)
template <class Net>
static int nf_paper_net_selftest_dw_tables() {
    constexpr int NX = nf_net_n_xyz<Net>, NG = nf_net_dw_groups<Net>;
    const long entries = 2L * 256 * 64 + (long)NX * 65536 + 128L * 272 + 2L * 128 * 128 + 4L * 128 + 4L * 256 + (NX + 1) * 256 + 3 * 128 + 4;
    NfDwGroup groups[NG];
    nf_paper_net_build_dw_groups<Net>(groups);
    int rc = nf_check_dw_groups(groups, NG, Net::SLAB_FLOATS, entries);
    if (rc) return rc;
    // the plan at the training sizes: one workgroup per CU at most, and the reduction can describe the short groups
    for (int64_t n : {(int64_t)131072, (int64_t)262144, (int64_t)259969, (int64_t)512}) {
        int first[NF_DW_MAX_GROUPS + 1];
        const int most = nf_dw_plan_groups(groups, NG, n, first);
        NfReduceAlt alt;
        if (first[NG] > 256 || most < 1 || !nf_dw_reduce_alt(groups, NG, most, &alt)) return -200;
        for (int i = 0; i < NG; ++i)
            if ((int64_t)groups[i].n_slices * groups[i].pts_per_slice < n || (groups[i].pts_per_slice & 15)) return -201;
    }
    return 0;
}

// =================================================================================================
// B3: reduce over slices + scatter to the reference parameter layout (state_dict order)
// =================================================================================================
// off[t]: first flat element of tensor t; blk[t]: first workgroup of tensor t (a workgroup handles 256 elements of ONE tensor, so
// the tensor id -- and with it the switch below -- is uniform: no per-element search, no divergence); tensor NPARAMS = d latent
template <class Net>
struct NfNetGradOffsets { int off[Net::NPARAMS + 2]; int blk[Net::NPARAMS + 2]; };

// elements of tensor `id`
template <class Net>
constexpr int nf_net_numel(int id) {
    const int r = nf_net_role<Net>(id);
    if (r & 1) return r == NF_R_ALPHA_B ? 1 : (r == NF_R_RGB_B ? 3 : (r < NF_R_ALPHA_B ? 256 : 128));   // biases
    return r == NF_R_XYZ0_W ? 256 * 171 : r == NF_R_XYZ3_W ? 256 * 427 : r < NF_R_ALPHA_W ? 65536 : r == NF_R_ALPHA_W ? 256
         : r == NF_R_DIR0_W ? 128 * Net::D0_COLS : r == NF_R_RGB_W ? 384 : 16384;
}
template <class Net>
constexpr int nf_net_numel_sum(int n) { return n == 0 ? 0 : nf_net_numel_sum<Net>(n - 1) + nf_net_numel<Net>(n - 1); }
static_assert(nf_net_numel_sum<NfPaperNet>(NfPaperNet::NPARAMS) == NfPaperNet::GRAD_PARAM_FLOATS, "paper model: tensor sizes");
static_assert(nf_net_numel_sum<NfSmallerNet>(NfSmallerNet::NPARAMS) == NfSmallerNet::GRAD_PARAM_FLOATS, "smaller model: tensor sizes");

// PE slot order -> reference columns; every folded column as (column sum of the layer's dZ) x (the constant it multiplied): expression and
// latent in layers_xyz.0 / .3, in layers_dir.0 the 16 near / far columns (and, D0_EXPR, the 76 expression columns);
// d latent = W0[:,139:171]^T db0 + W3[:,139:171]^T db3 (the latent code does not reach layers_dir.0)
template <class Net>
__device__ __forceinline__ void nf_paper_net_grad_unpack(const float* __restrict__ sum, const float* __restrict__ packed,
                                                         const float* __restrict__ cond, const NfNetGradOffsets<Net>& offs,
                                                         float* __restrict__ grads) {
    constexpr int CS_FEAT = Net::CS_L0 + 256 * nf_net_n_xyz<Net>;
    const float* cvec = cond + Net::B_CVEC;
    const float* dvec = cond + Net::B_DVEC;
    int t = 0;
    while ((int)blockIdx.x >= offs.blk[t + 1]) ++t;                 // uniform
    const int local = ((int)blockIdx.x - offs.blk[t]) * 256 + (int)threadIdx.x;
    if (t == Net::NPARAMS) {
        // d latent_j = sum_n W0[n][139+j] db0[n] + W3[n][139+j] db3[n]: the one workgroup of this "tensor" used to run 32 threads through
        // 256 dependent trips -- the longest path of the launch.  All 256 threads: thread (q, j) sums n = 32 q .. 32 q + 31, the eight
        // partial sums of a j are added in a fixed order (deterministic; the association differs from a single running sum).
        __shared__ float part[8][32];
        const int j = (int)threadIdx.x & 31, q = (int)threadIdx.x >> 5;
        const float* w0 = packed + Net::OFF_WC0 + 76 + j;
        const float* w3 = packed + Net::OFF_WC3 + 76 + j;
        float v = 0.f;
#pragma unroll 8
        for (int n = 32 * q; n < 32 * q + 32; ++n) v += w0[n * Net::NCOND] * sum[Net::CS_L0 + n] + w3[n * Net::NCOND] * sum[Net::CS_L0 + 768 + n];
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
    switch (nf_net_role<Net>(t)) {
        case 0: {  // layers_xyz.0.weight [256][171]
            const int n = local / 171, col = local - 171 * n;
            v = col < 63 ? sum[Net::G_L0 + n * 64 + nfl::pe_col_to_slot(col)] : sum[Net::CS_L0 + n] * cvec[col - 63];
        } break;
        case 1: v = sum[Net::CS_L0 + local]; break;
        case 2: v = sum[Net::G_L1 + local]; break;
        case 3: v = sum[Net::CS_L0 + 256 + local]; break;
        case 4: v = sum[Net::G_L2 + local]; break;
        case 5: v = sum[Net::CS_L0 + 512 + local]; break;
        case 6: {  // layers_xyz.3.weight [256][427] = [pe 63 | cond 108 | hidden 256]
            const int n = local / 427, col = local - 427 * n;
            v = col < 63 ? sum[Net::G_L3A + n * 64 + nfl::pe_col_to_slot(col)]
                         : (col < 171 ? sum[Net::CS_L0 + 768 + n] * cvec[col - 63] : sum[Net::G_L3B + n * 256 + (col - 171)]);
        } break;
        case 7: v = sum[Net::CS_L0 + 768 + local]; break;
        case 8: v = sum[Net::G_L4 + local]; break;
        case 9: v = sum[Net::CS_L0 + 1024 + local]; break;
        case NF_R_L5_W: if constexpr (Net::HAS_L5) v = sum[Net::G_L5 + local]; break;
        case NF_R_L5_W + 1: v = sum[Net::CS_L0 + 1280 + local]; break;
        case NF_R_FEAT_W: v = sum[Net::G_FEAT + local]; break;
        case NF_R_FEAT_B: v = sum[CS_FEAT + local]; break;
        case NF_R_ALPHA_W: v = sum[Net::G_ALPHA + 3 * 256 + local]; break;   // fc_alpha.weight [1][256] = row 3 (d sigma) of d_raw^T feat
        case NF_R_ALPHA_B: v = sum[Net::CS_RGB + 3]; break;
        case NF_R_DIR0_W: {  // layers_dir.0.weight [128][D0_COLS] = [feat 256 | PE4(rd_z, near, far) 24 (| expr/3 76)]
            const int n = local / Net::D0_COLS, col = local - Net::D0_COLS * n;
            if (col < 256) v = sum[Net::G_D0A + n * 256 + col];
            else if (!Net::D0_EXPR || col < 280) {
                const int q = col - 256, f = q / 6, rem = q - 6 * f, sc = rem / 3, comp = rem - 3 * sc;
                v = comp == 0 ? sum[Net::G_D0B + n * 16 + 4 * f + sc] : sum[Net::CS_D0 + n] * dvec[4 * f + 2 * sc + (comp - 1)];
            } else v = sum[Net::CS_D0 + n] * cvec[col - 280];
        } break;
        case NF_R_DIR0_B: v = sum[Net::CS_D0 + local]; break;
        case NF_R_DIR1_W: v = sum[Net::G_D1 + local]; break;
        case NF_R_DIR1_W + 1: v = sum[Net::CS_D0 + 128 + local]; break;
        case NF_R_DIR2_W: v = sum[Net::G_D2 + local]; break;
        case NF_R_DIR2_W + 1: v = sum[Net::CS_D0 + 256 + local]; break;
        case 22: case 23: v = 0.f; break;                      // layers_dir.3: never used (Quirk Q3)
        case NF_R_RGB_W: v = sum[Net::G_RGB + local]; break;   // fc_rgb.weight [3][128]
        case NF_R_RGB_B: v = sum[Net::CS_RGB + local]; break;
    }
    grads[offs.off[t] + local] = v;
}

// `unpack` = the family's k_*_grad_unpack
template <class Net, class Unpack>
static inline void nf_paper_net_reduce_unpack(Unpack unpack, const float* slabs, int ns, const NfReduceAlt& alt, float* sum,
                                              const float* packed, const float* cond, float* grads, hipStream_t s) {
    hipLaunchKernelGGL((k_grad_reduce<Net::MODEL>), dim3(512), dim3(256), 0, s, slabs, ns, (int)Net::SLAB_FLOATS, sum, alt);
    NfNetGradOffsets<Net> offs;
    offs.off[0] = offs.blk[0] = 0;
    for (int i = 0; i <= Net::NPARAMS; ++i) {                         // the tensors, then the 32 latent-code gradients
        const int numel = i < Net::NPARAMS ? nf_net_numel<Net>(i) : 32;
        offs.off[i + 1] = offs.off[i] + numel;
        offs.blk[i + 1] = offs.blk[i] + (numel + 255) / 256;
    }
    hipLaunchKernelGGL(unpack, dim3(offs.blk[Net::NPARAMS + 1]), dim3(256), 0, s, sum, packed, cond, offs, grads);
}
