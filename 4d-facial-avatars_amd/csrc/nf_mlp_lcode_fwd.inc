// The exact-f32 inference forward of the second model family from rays, as text: the body of k_lcode_mlp_fwd (nf_mlp_lcode.hip) and,
// with NF_LCODE_SIGMA_ONLY 1, of the density-only k_lcode_mlp_sigma (nf_mlp_lcode_sigma.hip), which ends with fc_alpha -- the layer
// behind layers_xyz.2 in this family's image -- and writes one float per point to `raw`.  Included once, as the statements of a
// kernel with the parameters (packed, cond, ro, rd, rd_view, z, n_points, S, raw) and the template parameter NT, behind the
// declaration of the workgroup's `lds`.  Text and not a function: the full kernel compiles to the code it had when this stood in it.
    using namespace nlc;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int64_t p0 = ((int64_t)blockIdx.x * NF_MLP_WAVES + wave) * (16 * NT);
    if (p0 >= n_points) return;
    f32x4* act4 = lds + wave * (16 * NT * 64);
    f32x4 pe[NT][4];
    f32x4 dirf[NT][1];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int64_t p = p0 + 16 * t + c;
        if (p >= n_points) p = n_points - 1;
        const int64_t ray = p / S;
        const float zz = z[p];
        const float px = nf_add(ro[ray * 3 + 0], nf_mul(rd[ray * 3 + 0], zz));
        const float py = nf_add(ro[ray * 3 + 1], nf_mul(rd[ray * 3 + 1], zz));
        const float pz = nf_add(ro[ray * 3 + 2], nf_mul(rd[ray * 3 + 2], zz));
        nf_encode_point(px, py, pz, g, pe[t]);
        float s, cs;
        nf_sincos(nf_mul(rd_view[ray * 3 + 2], (float)(1 << g)), &s, &cs);
        dirf[t][0] = (f32x4){s, cs, 0.0f, 0.0f};
    }
    f32x4 acc[NT][16];
    // Layer-streamed form (nf_mlp_stream.h; same form as the paper model's nf_paper_net_body, nf_mlp_paper_net.h).  layers_xyz.2's output feeds fc_alpha AND
    // fc_feat: fc_alpha's tail stores nothing (NO_ST = 0), so fc_feat reads the same slab again.
    NfStream<NT> st;
    f32x4 bj[NT];
    float sigma_raw[NT];
    const NfW Wi = nf_w_image(packed, PACKED), Ci = nf_w_image(cond, COND_FLOATS);
#define NF_PE_B(J_) do { _Pragma("unroll") for (int t = 0; t < NT; ++t) bj[t] = pe[t][J_]; } while (0)
    nf_load_bias<16>(st.bias, Ci, B_L1, lane);                           // layer1: no activation (M:609)
    {
        f32x4 w[16];
        nf_load_w16<16>(w, Wi, OFF_L1 / 4, lane);
        NF_PE_B(0); nf_chunk<NT, 16, true>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L1 / 4 + 1 * 16 * 64, lane);
        NF_PE_B(1); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L1 / 4 + 2 * 16 * 64, lane);
        NF_PE_B(2); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);
        nf_load_w16<16>(w, Wi, OFF_L1 / 4 + 3 * 16 * 64, lane);
        NF_PE_B(3); nf_tail<NT, 16, 16, 16, 1>(acc, w, bj, st, Wi, OFF_X0 / 4, Ci, B_X0, act4, lane);
    }
#undef NF_PE_B
    nf_seg_lds<NT, 16, true, false>(acc, st, Wi, OFF_X0 / 4, 16, act4, lane);       // reads layer1's output as stored
    nf_pending_b<NT, false>(bj, st);
    nf_tail<NT, 16, 16, 16, 1>(acc, st.wb, bj, st, Wi, OFF_X1 / 4, Ci, B_X1, act4, lane);
    nf_seg_lds<NT, 16, true, true>(acc, st, Wi, OFF_X1 / 4, 16, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 16, 16, 16, 1>(acc, st.wb, bj, st, Wi, OFF_X2 / 4, Ci, B_X2, act4, lane);
    nf_seg_lds<NT, 16, true, true>(acc, st, Wi, OFF_X2 / 4, 16, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 16, 16, 1, 1>(acc, st.wb, bj, st, Wi, OFF_ALPHA / 4, Ci, B_ALPHA, act4, lane);
    nf_seg_lds<NT, 1, true, true>(acc, st, Wi, OFF_ALPHA / 4, 16, act4, lane);      // fc_alpha(x)
    nf_pending_b<NT, true>(bj, st);
#if NF_LCODE_SIGMA_ONLY
    // density only: fc_alpha's last chunk with nothing fetched behind it (same MFMAs, same order as nf_tail issues); `raw` is sigma[n_points]
    nf_chunk<NT, 1, false>(acc, st.wb, bj, st.bias);
    if (g == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int64_t p = p0 + 16 * t + c;
            if (p < n_points) raw[p] = acc[t][0].x;
        }
    }
#else
    nf_tail<NT, 1, 0, 16, 1>(acc, st.wb, bj, st, Wi, OFF_FEAT / 4, Ci, B_FEAT, act4, lane);
#pragma unroll
    for (int t = 0; t < NT; ++t) sigma_raw[t] = acc[t][0].x;
    nf_seg_lds<NT, 16, true, true>(acc, st, Wi, OFF_FEAT / 4, 16, act4, lane);      // feat = relu(fc_feat(x)): the ReLU is the reader's
    nf_pending_b<NT, true>(bj, st);
    nf_tail<NT, 16, 16, 8, 1>(acc, st.wb, bj, st, Wi, OFF_DIR / 4, Ci, B_DIR, act4, lane);
    {
        f32x4 wd[16];
        nf_load_w16<8>(wd, Wi, OFF_DIR / 4 + 16 * 8 * 64, lane);                    // the dir-slot chunk's weights, a layer ahead
        nf_seg_lds<NT, 8, true, true>(acc, st, Wi, OFF_DIR / 4, 16, act4, lane);    // relu(layers_dir.0([feat | dir]))
        nf_pending_b<NT, true>(bj, st);
        nf_chunk<NT, 8, false>(acc, st.wb, bj, st.bias);
#pragma unroll
        for (int t = 0; t < NT; ++t) bj[t] = dirf[t][0];
        nf_tail<NT, 8, 8, 1, 1>(acc, wd, bj, st, Wi, OFF_RGB / 4, Ci, B_RGB, act4, lane);
    }
    nf_seg_lds<NT, 1, true, true>(acc, st, Wi, OFF_RGB / 4, 8, act4, lane);
    nf_pending_b<NT, true>(bj, st);
    nf_chunk<NT, 1, false>(acc, st.wb, bj, st.bias);
    if (g == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int64_t p = p0 + 16 * t + c;
            if (p < n_points) reinterpret_cast<f32x4*>(raw)[p] = (f32x4){acc[t][0].x, acc[t][0].y, acc[t][0].z, sigma_raw[t]};
        }
    }
#endif
