#include <type_traits>
#include "nf_mlp_bf16_machinery.inc"

// Body of the split-bf16 fused forward of the second model family (included once per translation unit with NFB_SAVE = 0 / 1
// and NFB_KERNEL_NAME set; separate translation units for the same reason as nf_mlp_bf16_kernel.inc).
// NFB_SAVE: training forward -- every layer output also goes to `saved` (f32 sections nlc::S_*, the layout of the exact-f32
// training forward) plus the ReLU bit masks the split-bf16 backward chain reads (nlc::S_MASK).
__global__ void __launch_bounds__(256, 1)
NFB_KERNEL_NAME(const char* __restrict__ wstream, const float* __restrict__ cond, const float* __restrict__ ro,
                const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z, int64_t n_points, int S,
                float* __restrict__ raw, float* __restrict__ saved) {
    using namespace nlc;
    constexpr bool SAVE = NFB_SAVE != 0;
    __shared__ __attribute__((aligned(16))) char lds[NFB_LDS_BYTES];
    NfbCtx cx;
    cx.lane = threadIdx.x & 63;
    cx.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cx.lds = lds;
    nfb_ctx_stream(cx, wstream, (unsigned)nfb::STREAM_BF16 * 2u);
    const int h = cx.lane >> 5, c = cx.lane & 31;
    const int64_t p_tile = ((int64_t)blockIdx.x * 4 + cx.wave) * 32;                 // first point of this wave's tile
    const int64_t p_raw = p_tile + c;
    const int64_t p = p_raw < n_points ? p_raw : n_points - 1;       // clamp: every wave must reach every barrier
    const float* bias = reinterpret_cast<const float*>(lds + NFB_NBUF * NFB_STAGE_BYTES);
    // per-layer weight scales of the fp16 instantiation (see nf_mlp_bf16_kernel.inc / nf_mlp_f16.hip); constant 1 for bf16
#if NFB_F16
    const float* __restrict__ wscale = reinterpret_cast<const float*>(wstream + (size_t)nfb::STREAM_BF16 * 2);
    constexpr float ACT = (float)(1 << NFB_ACT_SHIFT);
    float wsc[2 * nfb::NL];
#pragma unroll
    for (int i = 0; i < 2 * nfb::NL; ++i) wsc[i] = wscale[i];
#pragma unroll
    for (int i = 0; i < 2 * nfb::NL; ++i) asm volatile("" : "+s"(wsc[i]));
#define SC(L_) wsc[L_]
#define INV(L_) wsc[nfb::NL + (L_)]
#define OUT_INV(L_) (wsc[nfb::NL + (L_)] * (1.0f / ACT))
#define NFB_TO_OPERANDS(L_, acc_, NO_, RELU_) nfb_to_operands_f16<NO_, RELU_>(acc_, bh, bl, 4, INV(L_), SC(L_) * (65504.0f / ACT))
#else
#define NFB_TO_OPERANDS(L_, acc_, NO_, RELU_) nfb_to_operands<NO_, RELU_>(acc_, bh, bl, 4, 1.0f)
    constexpr float ACT = 1.0f;
#define SC(L_) 1.0f
#define INV(L_) 1.0f
#define OUT_INV(L_) 1.0f
#endif

    // prologue DMA: bias table (10 KiB of the padded cond buffer), stages 0..2
    nfb_issue<NFB_BIAS_BLOCKS>(cx, reinterpret_cast<const char*>(cond) + cx.lane * 16, 0, NFB_NBUF * NFB_STAGE_BYTES);
    nfb_issue_w<nfb::stage_nblk(0)>(cx, nfb::stage_blk0(0), 0);
    nfb_issue_w<nfb::stage_nblk(1)>(cx, nfb::stage_blk0(1), NFB_STAGE_BYTES);
    nfb_issue_w<nfb::stage_nblk(2)>(cx, nfb::stage_blk0(2), 2 * NFB_STAGE_BYTES);

    bf16x8 bh[20], bl[20];                                            // [0..4): PE k-steps
    bf16x8 dh, dl;                                                    // dir k-step
    {
        const int64_t ray = p / S;
        const float zz = z[p];
        const float px = nf_add(ro[ray * 3 + 0], nf_mul(rd[ray * 3 + 0], zz));
        const float py = nf_add(ro[ray * 3 + 1], nf_mul(rd[ray * 3 + 1], zz));
        const float pz = nf_add(ro[ray * 3 + 2], nf_mul(rd[ray * 3 + 2], zz));
        // (four explicit calls, not a loop: with the training stores inlined the optimizer refuses to fully unroll a loop of
        // this size, and a rolled loop would index the operand arrays dynamically, i.e. put them in scratch memory)
        auto pe_step = [&](auto s_tag) {
            constexpr int s = decltype(s_tag)::value;
            float x[8];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int pr = 16 * h + 4 * s + jj;                   // pair index (nfb::pe_col)
                const int freq = pr / 3, comp = pr - 3 * freq;
                const float v = comp == 0 ? px : (comp == 1 ? py : pz);
                float sn, cs;
                nf_sincos(nf_mul(v, (float)(1 << (freq < 10 ? freq : 0))), &sn, &cs);
                x[2 * jj] = sn;
                x[2 * jj + 1] = cs;
            }
            if (s == 3 && h == 1) { x[4] = px; x[5] = py; x[6] = pz; x[7] = 0.f; }
            if (NFB_F16) {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] *= ACT;
            }
            nfb_split(x, bh[s], bl[s]);
            if (SAVE && p_raw < n_points) {
                // saved PE uses the f32 kernels' slot order (nfl::pe_slot_to_col): the (sin, cos) of two consecutive pairs --
                // this lane's x[0..3] and x[4..7] -- are 4 consecutive slots there (raw xyz + pad: slots 60..63), so two
                // 16-byte stores per k-step instead of eight scalar ones
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int col = nfb::pe_col(s, h, 4 * q);
                    const int slot0 = nfl::pe_col_to_slot(col);
                    *reinterpret_cast<f32x4*>(saved + (int64_t)S_PE * nfb_pad32(n_points) + p * 64 + slot0) =          // true values: 1/ACT is exact
                        (f32x4){x[4 * q] * (1.0f / ACT), x[4 * q + 1] * (1.0f / ACT), x[4 * q + 2] * (1.0f / ACT), x[4 * q + 3] * (1.0f / ACT)};
                }
            }
        };
        pe_step(std::integral_constant<int, 0>{});
        pe_step(std::integral_constant<int, 1>{});
        pe_step(std::integral_constant<int, 2>{});
        pe_step(std::integral_constant<int, 3>{});
        const float dzv = rd_view[ray * 3 + 2];                       // Quirk Q1: "direction" = (rd_z, near, far)
        float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            float sn, cs;
            nf_sincos(nf_mul(dzv, (float)(1 << (2 * h + jj))), &sn, &cs);
            x[2 * jj] = sn * ACT;
            x[2 * jj + 1] = cs * ACT;
        }
        nfb_split(x, dh, dl);
        if (SAVE && p_raw < n_points) {                              // dir slots of the f32 kernels: group g = frequency, (sin, cos, 0, 0)
            float* d = saved + (int64_t)S_DIRF * nfb_pad32(n_points) + p * 16;
            *reinterpret_cast<f32x4*>(d + 4 * (2 * h)) = (f32x4){x[0] * (1.0f / ACT), x[1] * (1.0f / ACT), 0.f, 0.f};
            *reinterpret_cast<f32x4*>(d + 4 * (2 * h + 1)) = (f32x4){x[2] * (1.0f / ACT), x[3] * (1.0f / ACT), 0.f, 0.f};
        }
    }
    nfb_wait_vm<nfb::inflight_after(-1)>();                            // bias + stage 0 landed (later stages may be in flight)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#if NFB_F16
    {
        // bias table scaled once per workgroup, in LDS (see nf_mlp_bf16_kernel.inc): layer l of the stream <-> its bias section
        float* bw = const_cast<float*>(bias);
        const int t = threadIdx.x;
        bw[B_L1 + t] *= SC(0);
        bw[B_X0 + t] *= SC(1);
        bw[B_X1 + t] *= SC(2);
        bw[B_X2 + t] *= SC(3);
        bw[B_FEAT + t] *= SC(5);
        if (t < 16) bw[B_ALPHA + t] *= SC(4);
        if (t < 128) bw[B_DIR + t] *= SC(6);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
#endif

    f32x16 accA[8];
    f32x16 (&accB)[8] = accA;          // (one accumulator set; the two names only keep the layer list below readable)
#if NFB_SAVE
    // training: the previous layer's output (= this layer's operands bh / bl[4..]) leaves as the dW kernel's fragment stream from
    // inside the K loop (transposing MFMAs, nf_mlp_bf16_machinery.inc); sections are n_pad = n_points rounded up to 32 points long
    bf16x8 sel[2];
    nfb_sel_operands(sel, cx.lane);
#endif
    const int64_t n_pad = nfb_pad32(n_points);
    bf16x8 th[20], tl[20];
    const bool live = p_raw < n_points;
    // layer epilogue: (training: true outputs, ReLU, bit masks,) accumulators -> operands of the next layer (slots 4..19; PE stays in 0..3)
#define NFB_LC_FINISH(L_, acc_, NO_, RELU_, MASK_)                                                       \
    do {                                                                                                 \
        /* training: the ReLU decisions as bit masks for the backward chain (from the raw accumulators: [x > 0] is scale-free) */ \
        if (SAVE && (RELU_) && live) nfb_save_mask<NO_>(acc_, saved + (int64_t)S_MASK * n_pad, MASK_, n_points, p, h); \
        NFB_TO_OPERANDS(L_, acc_, NO_, RELU_);                                                           \
    } while (0)
    // layer L_ into acc_; training: the NOP_ tiles of the layer before (operand k-steps 4.. of bh / bl) are streamed to section PSEC_
#if NFB_SAVE
#define NFB_LC_RUN(L_, acc_, oh_, ol_, NOP_, prev_, PSEC_)                                               \
    do {                                                                                                 \
        const NfbStreamTarget tg_ = nfb_stream_target(saved + (int64_t)(PSEC_) * n_pad, NOP_, p_tile, n_pad, cx.lane); \
        NFB_LAYER_STREAMING(L_, acc_, oh_, ol_, NOP_, bh, bl, sel, tg_);                                 \
    } while (0)
#else
#define NFB_LC_RUN(L_, acc_, oh_, ol_, NOP_, prev_, PSEC_) NFB_LAYER(L_, acc_, oh_, ol_)
#endif
    // ---- layer1: PE -> 256, no activation (M:609) -----------------------------------------------------------------------
    nfb_init_bias<8>(accA, bias + B_L1, h);
    NFB_LAYER(0, accA, bh, bl);
    NFB_LC_FINISH(0, accA, 8, false, 0);
#define NFB_LC_HIDDEN(L_, acc_, BIAS_, MASK_, prev_, PSEC_)                          \
    do {                                                                             \
        nfb_init_bias<8>(acc_, bias + (BIAS_), h);                                   \
        _Pragma("unroll") for (int s = 0; s < 16; ++s) { th[s] = bh[4 + s]; tl[s] = bl[4 + s]; } \
        NFB_LC_RUN(L_, acc_, th, tl, 8, prev_, PSEC_);                               \
        NFB_LC_FINISH(L_, acc_, 8, true, MASK_);                                     \
    } while (0)
    NFB_LC_HIDDEN(1, accB, B_X0, 0, accA, S_L1);
    NFB_LC_HIDDEN(2, accA, B_X1, 1, accB, S_X0);
    NFB_LC_HIDDEN(3, accB, B_X2, 2, accA, S_X1);
    // ---- fc_alpha(x) (one tile, row 0), then feat = relu(fc_feat(x)) on the same operands -----------------------------------
    // (training: x2, the output of layers_xyz.2 = these operands, is streamed from inside fc_feat's K loop)
#pragma unroll
    for (int s = 0; s < 16; ++s) { th[s] = bh[4 + s]; tl[s] = bl[4 + s]; }
    nfb_zero(accA[0]);
    if (h == 0) accA[0][0] = bias[B_ALPHA];
    NFB_LAYER(4, accA, th, tl);
    const float sigma_raw = accA[0][0] * OUT_INV(4);
    nfb_init_bias<8>(accA, bias + B_FEAT, h);
    NFB_LC_RUN(5, accA, th, tl, 8, accB, S_X2);
    NFB_LC_FINISH(5, accA, 8, true, 3);
#undef NFB_LC_HIDDEN
    // ---- layers_dir.0: 16 feat k-steps + dir k-step + 1 zero k-step -> 128, ReLU -----------------------------------------
    nfb_init_bias<4>(accB, bias + B_DIR, h);
#pragma unroll
    for (int s = 0; s < 16; ++s) { th[s] = bh[4 + s]; tl[s] = bl[4 + s]; }
    th[16] = dh; tl[16] = dl;
#pragma unroll
    for (int s = 17; s < nfb::KS[6]; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) { th[s][j] = (nfb_elt)0.f; tl[s][j] = (nfb_elt)0.f; }
    NFB_LC_RUN(6, accB, th, tl, 8, accA, S_FEAT);
    NFB_LC_FINISH(6, accB, 4, true, 4);
#undef NFB_LC_FINISH
    // ---- fc_rgb ---------------------------------------------------------------------------------------------------------
    nfb_zero(accA[0]);
#pragma unroll
    for (int s = 0; s < 8; ++s) { th[s] = bh[4 + s]; tl[s] = bl[4 + s]; }
    NFB_LC_RUN(7, accA, th, tl, 4, accB, S_DIR);
#undef NFB_LC_RUN
    if (h == 0 && p_raw < n_points) {
        const float inv = OUT_INV(7);
        const f32x4 o = {accA[0][0] * inv + bias[B_RGB + 0], accA[0][1] * inv + bias[B_RGB + 1], accA[0][2] * inv + bias[B_RGB + 2], sigma_raw};
        reinterpret_cast<f32x4*>(raw)[p_raw] = o;
    }
#if NFB_F16
    if (live && h == 0 && !(fabsf(sigma_raw) < INFINITY))                // range guard, see nf_mlp_bf16_kernel.inc
        atomicOr(reinterpret_cast<unsigned*>(const_cast<float*>(wscale)) + NF_F16_FLAG_WORD, 1u);
#endif
#undef SC
#undef INV
#undef OUT_INV
#undef NFB_TO_OPERANDS
}

