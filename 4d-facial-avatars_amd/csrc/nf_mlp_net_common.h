// What the exact-f32 networks of both shapes share -- the paper-shaped one (nf_mlp_paper_net.h, nf_mlp_paper_net_bwd.h) and the second
// family's (nf_mlp_lcode_net.h, nf_mlp_lcode_net_bwd.h): the input fragments of one wave, the `raw` store, and the parts of the layer
// stream (nf_mlp_stream.h) that do not depend on the layer list -- the PE layer, the saving forward's layer step and the front, layer
// step and end of the dX chain.  The stream parts are text (macros over the kernel's locals and a traits struct `Net`: they declare or
// use acc / st / bj / m64 / sec / masks); the family's layer list stays in the family's kernel.
#pragma once
#include "nf_mlp_dev.h"
#include "nf_mlp_stream.h"

// =================================================================================================
// inputs and outputs of one wave
// =================================================================================================
// from rays: pts = ro + rd*z (T:78), PE fragments, dir fragment
template <int NT>
__device__ __forceinline__ void nf_net_inputs(f32x4 (&pe)[NT][4], f32x4 (&dirf)[NT][1], int64_t p0, int64_t n_points, int S, int lane,
                                              const float* __restrict__ ro, const float* __restrict__ rd,
                                              const float* __restrict__ rd_view, const float* __restrict__ z) {
    const int g = lane >> 4, c = lane & 15;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int64_t p = p0 + 16 * t + c;
        if (p >= n_points) p = n_points - 1;
        const int64_t ray = p / S;
        const float zz = z[p];
        const float dx = rd[ray * 3 + 0], dy = rd[ray * 3 + 1], dz = rd[ray * 3 + 2];
        const float px = nf_add(ro[ray * 3 + 0], nf_mul(dx, zz));
        const float py = nf_add(ro[ray * 3 + 1], nf_mul(dy, zz));
        const float pz = nf_add(ro[ray * 3 + 2], nf_mul(dz, zz));
        nf_encode_point(px, py, pz, g, pe[t]);
        float s, cs;
        nf_sincos(nf_mul(rd_view[ray * 3 + 2], (float)(1 << g)), &s, &cs);   // Quirk Q1: "direction" = (rd_z, near, far)
        dirf[t][0] = (f32x4){s, cs, 0.0f, 0.0f};
    }
}

// from PRE-ENCODED rows x87 (P, 87) = [PE10(xyz) (63) | PE4(dirs) (24)]: the PE fragments in slot order and the 24 direction columns
// in reference order as two register chunks
template <int NT>
__device__ __forceinline__ void nf_net_inputs_encoded(f32x4 (&pe)[NT][4], f32x4 (&dirf)[NT][2], int64_t p0, int64_t n_points, int lane,
                                                      const float* __restrict__ x87) {
    const int g = lane >> 4, c = lane & 15;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int64_t p = p0 + 16 * t + c;
        if (p >= n_points) p = n_points - 1;
        const float* row = x87 + p * 87;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = nfl::pe_slot_to_col(16 * j + 4 * g + r);
                v[r] = col >= 0 ? row[col] : 0.0f;
            }
            pe[t][j] = (f32x4){v[0], v[1], v[2], v[3]};
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = 16 * j + 4 * g + r;
                v[r] = s < 24 ? row[63 + s] : 0.0f;
            }
            dirf[t][j] = (f32x4){v[0], v[1], v[2], v[3]};
        }
    }
}

// rgb_raw / sigma_raw of the wave's points -> out (n_points, 4): lane group 0 holds them
template <int NT>
__device__ __forceinline__ void nf_net_store_raw(const f32x4 (&acc)[NT][16], const float (&sigma_raw)[NT], int64_t p0, int64_t n_points,
                                                 int lane, float* __restrict__ out) {
    const int g = lane >> 4, c = lane & 15;
    if (g == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int64_t p = p0 + 16 * t + c;
            if (p < n_points) reinterpret_cast<f32x4*>(out)[p] = (f32x4){acc[t][0].x, acc[t][0].y, acc[t][0].z, sigma_raw[t]};
        }
    }
}

// =================================================================================================
// forward stream
// =================================================================================================
#define NF_NET_PE_B(J_) do { _Pragma("unroll") for (int t = 0; t < NT; ++t) bj[t] = pe[t][J_]; } while (0)
// the network's first layer : PE(64 slots) -> 256, four register chunks; ends in the tail that fetches the next 256-wide layer
#define NF_NET_PE_LAYER(B_, OFF_, OFF_NEXT_, B_NEXT_)                                                         \
    do {                                                                                                      \
        nf_load_bias<16>(st.bias, Ci, B_, lane);                                                              \
        f32x4 w[16];                                                                                          \
        nf_load_w16<16>(w, Wi, (OFF_) / 4, lane);                                                             \
        NF_NET_PE_B(0); nf_chunk<NT, 16, true>(acc, w, bj, st.bias);                                          \
        nf_load_w16<16>(w, Wi, (OFF_) / 4 + 1 * 16 * 64, lane);                                               \
        NF_NET_PE_B(1); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);                                         \
        nf_load_w16<16>(w, Wi, (OFF_) / 4 + 2 * 16 * 64, lane);                                               \
        NF_NET_PE_B(2); nf_chunk<NT, 16, false>(acc, w, bj, st.bias);                                         \
        nf_load_w16<16>(w, Wi, (OFF_) / 4 + 3 * 16 * 64, lane);                                               \
        NF_NET_PE_B(3); nf_tail<NT, 16, 16, 16, 1>(acc, w, bj, st, Wi, (OFF_NEXT_) / 4, Ci, B_NEXT_, act4, lane); \
    } while (0)

// ---- the saving (training) forward: what the backward needs is produced where the slab is READ.  Locals: saved, p0, n, sec ------
// the last chunk's fragment (+ its mask bits), then the finished mask words of ReLU layer MASKL_ (the layer whose output was just consumed)
#define NF_NET_SAVE_PENDING(RELU_, MASKL_, NCH_)                                                    \
    do {                                                                                            \
        nf_pending_b<NT, RELU_>(bj, st);                                                            \
        if ((MASKL_) >= 0) {                                                                        \
            nf_mask_bits<NT>(m64, st.bp, (NCH_) - 2);                                               \
            nf_mask_bits<NT>(m64, bj, (NCH_) - 1);                                                  \
            _Pragma("unroll") for (int t = 0; t < NT; ++t)                                          \
                if (p0 + 16 * t < n)                                                                \
                    *nf_mask_ptr<Net::S_MASK>(saved, n, (MASKL_) >= 0 ? (MASKL_) : 0, (p0 >> 4) + t, lane) = make_uint2((uint32_t)m64[t], (uint32_t)(m64[t] >> 32)); \
        }                                                                                           \
    } while (0)
// one 256-wide layer from the slab: the slab = section SEC_ (ReLU layer MASKL_, or -1: as stored) is copied out and consumed
#define NF_NET_SAVE_LAYER256(OFF_, FIRST_, SEC_, MASKL_, OFF_NEXT_, B_NEXT_, NO_NEXT_, NEXT_B_)                           \
    do {                                                                                                                   \
        NfCopyH<64, 4, ((MASKL_) >= 0)> cs{act4, sec(SEC_, 256), lane, 8, {}};                                             \
        cs.prime();                                                                                                        \
        _Pragma("unroll") for (int t = 0; t < NT; ++t) m64[t] = 0;                                                         \
        nf_seg_lds<NT, 16, FIRST_, ((MASKL_) >= 0), ((MASKL_) >= 0)>(acc, st, Wi, OFF_, 16, act4, lane, cs, m64);          \
        NF_NET_SAVE_PENDING(((MASKL_) >= 0), MASKL_, 16);                                                                  \
        nf_tail<NT, 16, 16, NO_NEXT_, NEXT_B_>(acc, st.wb, bj, st, Wi, OFF_NEXT_, Ci, B_NEXT_, act4, lane);               \
    } while (0)

// =================================================================================================
// dX chain of one wave, on the forward kernels' streamed K loops (nf_seg_lds, nf_tail_dz): C = 0 is the C operand of a layer's first
// MFMAs, the copy of the slab to `dz` rides in the loops (whole lines through a range-checked descriptor), the layer boundary sits
// under the last chunk's MFMAs with the ReLU mask applied on the way to the slab, and a layer's two mask words (saved by the training
// forward) are fetched when its loop starts.  Parameters in scope: lds, packed_t, saved, d_raw, n_points, dz.
// =================================================================================================
// Setup, then d(last hidden layer's out) = d rgb . fc_rgb.weight, masked by that layer's ReLU MASKL_ (one register chunk); fetches the
// first slab layer (weights OFF_NEXT_, NO_NEXT_ output tiles).  Leaves frag_sig = the d-sigma register chunk for the family's list.
#define NF_NET_CHAIN_BEGIN(MASKL_, OFF_NEXT_, NO_NEXT_)                                                               \
    static_assert(NT == 2, "the copy schedule below is written for 32-point slabs");                                 \
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;                                                      \
    const int g = lane >> 4, c = lane & 15;                                                                          \
    const int64_t p0 = ((int64_t)blockIdx.x * NF_MLP_WAVES + wave) * (16 * NT);                                      \
    if (p0 >= n_points) return;                                                                                      \
    f32x4* act4 = lds + wave * (16 * NT * 64);                                                                       \
    const int64_t n = n_points;                                                                                      \
    const NfW Wi = nf_w_image(packed_t, Net::PACKED_T);                                                              \
    auto sec = [&](int zs, int width) { return nf_slab_copy(dz, zs, width, p0, n); };                                \
    auto masks = [&](int l, uint2 (&m)[NT]) {                                                                        \
        _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                               \
            m[t] = p0 + 16 * t < n ? *nf_mask_ptr<Net::S_MASK>(const_cast<float*>(saved), n, l, (p0 >> 4) + t, lane) : make_uint2(0u, 0u); \
    };                                                                                                               \
    f32x4 frag_rgb[NT][1], frag_sig[NT];                                                                             \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) {                                                                 \
        const int64_t p = p0 + 16 * t + c;                                                                           \
        f32x4 d = (f32x4){0.f, 0.f, 0.f, 0.f};                                                                       \
        if (p < n && g == 0) d = reinterpret_cast<const f32x4*>(d_raw)[p];                                           \
        frag_rgb[t][0] = (f32x4){d.x, d.y, d.z, 0.f};                                                                \
        frag_sig[t] = (f32x4){d.w, 0.f, 0.f, 0.f};                                                                   \
    }                                                                                                                \
    f32x4 acc[NT][16];                                                                                               \
    NfStream<NT> st;                                                                                                 \
    f32x4 bj[NT];                                                                                                    \
    uint64_t unused64[NT];                                                                                           \
    uint2 m[NT];                                                                                                     \
    _Pragma("unroll") for (int no = 0; no < 16; ++no) st.bias[no] = (f32x4){0.f, 0.f, 0.f, 0.f};                     \
    masks(MASKL_, m);                                                                                                \
    nf_zero_acc<NT, 8>(acc);                                                                                         \
    nf_mma_from_regs<NT, 8, 1>(acc, reinterpret_cast<const f32x4*>(packed_t) + Net::OFFT_RGB / 4, frag_rgb, lane);   \
    nf_apply_mask<NT, 8>(acc, m);                                                                                    \
    nf_store_act<NT, 8, false>(acc, act4, lane);                                                                     \
    nf_load_w16<NO_NEXT_>(st.wa, Wi, OFF_NEXT_, lane);                                                               \
    nf_read_b<NT>(st.b0, act4, lane, 0)
// one layer from the slab: the slab = dZ section ZSEC_ (W4_ float4 per row) is copied out and consumed; the output is masked by
// ReLU layer MASKL_ (-1: no activation) under the last chunk and becomes the next slab
#define NF_NET_CHAIN_LAYER(OFF_, NO_, NCH_, W4_, ZSEC_, MASKL_, OFF_NEXT_, NO_NEXT_)                                   \
    do {                                                                                                             \
        NfCopyH<W4_, 4, false> cs{act4, sec(ZSEC_, 4 * (W4_)), lane, (NCH_) / 2, {}};                                  \
        cs.prime();                                                                                                  \
        if ((MASKL_) >= 0) masks((MASKL_) >= 0 ? (MASKL_) : 0, m);                                                   \
        nf_seg_lds<NT, NO_, true, false, false>(acc, st, Wi, OFF_, NCH_, act4, lane, cs, unused64);                  \
        nf_pending_b<NT, false>(bj, st);                                                                             \
        nf_tail_dz<NT, NO_, NO_NEXT_, ((MASKL_) >= 0)>(acc, st.wb, bj, st, Wi, OFF_NEXT_, act4, lane, m);            \
    } while (0)
// the last section (the first layer's dZ, 256 wide) has no K loop behind it
#define NF_NET_CHAIN_END(ZSEC_)                                                                                      \
    do {                                                                                                             \
        const NfSlabCopy cp = sec(ZSEC_, 256);                                                                       \
        _Pragma("unroll 4") for (int k = 0; k < 16 * NT; ++k) nf_copy_rows<64>(act4, cp, k, lane);                   \
    } while (0)
