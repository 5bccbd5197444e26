// The family-independent text of the split-precision fused forward, included ONCE, as the first statements of the body of a
// family's __global__ kernel (nf_mlp_bf16_kernel.inc: paper model; nf_mlp_lcode_bf16_kernel.inc: second family).  It is text and
// not a function because the kernels are scheduled to the instruction: every one of them compiles to the code it had when this
// text stood in each kernel body (profiles/split_families_shared.md).  The kernel's parameters are the names used here (wstream,
// cond, ro, rd, rd_view, z, n_points, S, raw, saved).  The family provides, before the #include:
//   NFB_SAVE                   0 / 1: the training instantiation also fills `saved`
//   NfbSections                the sections of `saved` written here: S_PE, S_DIRF, S_MASK (nf_mlp_*bf16_common.h)
//   NFB_SCALE_BIASES(bw, t)    (NFB_F16) thread t's share of scaling the LDS bias table bw by SC(l), section by section
// What stands behind this file in the kernel body: the family's layer list, written with the macros defined at the end of this
// file, and NFB_STORE_RAW.
//
// ---- front: tile, scales, prologue DMA, input encoding, bias table -------------------------------------------------------------
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
    // per-layer weight scales 2^e (fp16 instantiation: stored behind the stream by the pack kernel; SC(l) multiplies the
    // bias the accumulators start from, INV(l) = 2^-e brings a layer's outputs back).  bf16: constant 1, folded away.
#if NFB_F16
    // activations travel as x * 2^NFB_ACT_SHIFT (keeps the fp16 `lo` parts of small activations in the normal range):
    // SC(l) = s_W(l) * 2^shift scales the bias, INV(l) = 1 / s_W(l) turns an accumulator into the NEXT layer's (pre-scaled)
    // operand, and OUT_INV(l) = INV(l) * 2^-shift into a true output
    // All 2 NL scales are fetched into SGPRs here, once: a scalar load inside the layer loop would need an s_waitcnt lgkmcnt(0),
    // and that counter is shared with the LDS reads of the weight ring.
    const float* __restrict__ wscale = reinterpret_cast<const float*>(wstream + (size_t)nfb::STREAM_BF16 * 2);
    constexpr float ACT = (float)(1 << NFB_ACT_SHIFT);
    float wsc[2 * nfb::NL];
#pragma unroll
    for (int i = 0; i < 2 * nfb::NL; ++i) wsc[i] = wscale[i];
#pragma unroll
    for (int i = 0; i < 2 * nfb::NL; ++i) asm volatile("" : "+s"(wsc[i]));          // pin: loaded now, kept in scalar registers
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
    if (NFB_LA > 2) nfb_issue_w<nfb::stage_nblk(2)>(cx, nfb::stage_blk0(2), 2 * NFB_STAGE_BYTES);

    // ---- inputs ---------------------------------------------------------------------------------------
    bf16x8 bh[20], bl[20];                                            // [0..4): PE k-steps (kept for a skip layer)
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
                    *reinterpret_cast<f32x4*>(saved + (int64_t)NfbSections::S_PE * nfb_pad32(n_points) + p * 64 + slot0) =          // true values: 1/ACT is exact
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
            float* d = saved + (int64_t)NfbSections::S_DIRF * nfb_pad32(n_points) + p * 16;
            *reinterpret_cast<f32x4*>(d + 4 * (2 * h)) = (f32x4){x[0] * (1.0f / ACT), x[1] * (1.0f / ACT), 0.f, 0.f};
            *reinterpret_cast<f32x4*>(d + 4 * (2 * h + 1)) = (f32x4){x[2] * (1.0f / ACT), x[3] * (1.0f / ACT), 0.f, 0.f};
        }
    }
    nfb_wait_vm<nfb::inflight_after(-1)>();                            // bias + stage 0 landed (later stages may be in flight)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#if NFB_F16
    {
        // the accumulators start from bias * (weight scale * activation scale): scaled HERE, once per workgroup and in LDS (ten
        // multiplies per thread), so that a layer's accumulator initialisation is four ds_read_b128 per tile and no vector
        // arithmetic (round 5: one v_mul per accumulator register, 1100 per wave)
        float* bw = const_cast<float*>(bias);
        const int t = threadIdx.x;
        NFB_SCALE_BIASES(bw, t);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
#endif

    f32x16 accA[8];
    f32x16 (&accB)[8] = accA;          // (one accumulator set; the two names only keep the layer lists readable)
#if NFB_SAVE
    // training: the previous layer's output (= this layer's operands bh / bl[4..]) leaves as the dW kernel's fragment stream from
    // inside the K loop (transposing MFMAs, nf_mlp_bf16_machinery.inc); sections are n_pad = n_points rounded up to 32 points long
    bf16x8 sel[2];
    nfb_sel_operands(sel, cx.lane);
#endif
    const int64_t n_pad = nfb_pad32(n_points);
    bf16x8 th[20], tl[20];
    const bool live = p_raw < n_points;

// ---- the layer macros of a family's layer list ------------------------------------------------------------------------------------
// layer epilogue: (training: the ReLU bit mask number MASK_,) accumulators -> operands of the next layer (slots 4..19, PE stays in 0..3)
#define NFB_FINISH(L_, acc_, NO_, RELU_, MASK_)                                                          \
    do {                                                                                                 \
        /* training: the ReLU decisions as bit masks for the backward chain (from the raw accumulators: [x > 0] is scale-free) */ \
        if (SAVE && (RELU_) && live) nfb_save_mask<NO_>(acc_, saved + (int64_t)NfbSections::S_MASK * n_pad, MASK_, n_points, p, h); \
        NFB_TO_OPERANDS(L_, acc_, NO_, RELU_);                                                           \
    } while (0)
// layer L_ into acc_; training: the NOP_ tiles of the layer before (they are operand k-steps 4.. of bh / bl) are streamed to
// section PSEC_ from inside its K loop
#if NFB_SAVE
#define NFB_RUN(L_, acc_, oh_, ol_, NOP_, prev_, PSEC_)                                                   \
    do {                                                                                                 \
        const NfbStreamTarget tg_ = nfb_stream_target(saved + (int64_t)(PSEC_) * n_pad, NOP_, p_tile, n_pad, cx.lane); \
        NFB_LAYER_STREAMING(L_, acc_, oh_, ol_, NOP_, bh, bl, sel, tg_);                                 \
    } while (0)
#else
#define NFB_RUN(L_, acc_, oh_, ol_, NOP_, prev_, PSEC_) NFB_LAYER(L_, acc_, oh_, ol_)
#endif
// a 256 -> 256 layer on the previous layer's output alone
#define NFB_HIDDEN_LAYER(L_, acc_, BIAS_, RELU_, MASK_, prev_, PSEC_)                \
    do {                                                                             \
        nfb_init_bias<8>(acc_, bias + (BIAS_), h);                                   \
        _Pragma("unroll") for (int s = 0; s < 16; ++s) { th[s] = bh[4 + s]; tl[s] = bl[4 + s]; } \
        NFB_RUN(L_, acc_, th, tl, 8, prev_, PSEC_);                                  \
        NFB_FINISH(L_, acc_, 8, RELU_, MASK_);                                       \
    } while (0)
// ---- back: rgb = tile 0, rows 0..2 of acc_ (fc_rgb, stream layer L_) + its bias at BIAS_; sigma_raw from the family's fc_alpha ----
#if NFB_F16
// Range guard, last line of defence (the first is the host's sampled pre-flight probe, nerf/ops.py: f16_preflight; the
// second the saturating ReLU of nfb_to_operands_f16): a non-finite density output -- fc_feat has no ReLU to saturate, so an
// overflow there reaches sigma as inf / NaN -- sets a sticky flag behind the stream (cleared by the pack kernel); the host polls
// it once per frame (check_f16_range) and raises.
#define NFB_RANGE_GUARD()                                                                                \
    if (live && h == 0 && !(fabsf(sigma_raw) < INFINITY))                                                \
        atomicOr(reinterpret_cast<unsigned*>(const_cast<float*>(wscale)) + NF_F16_FLAG_WORD, 1u)
#else
#define NFB_RANGE_GUARD() (void)0
#endif
// density-only kernels (NFB_SIGMA_ONLY, NFB_RUN_LAYERS): `raw` is sigma[n_points]; the layer list ends here
#define NFB_STORE_SIGMA()                                                                                \
    do {                                                                                                 \
        if (h == 0 && p_raw < n_points) raw[p_raw] = sigma_raw;                                          \
        NFB_RANGE_GUARD();                                                                               \
    } while (0)
#define NFB_STORE_RAW(L_, acc_, BIAS_)                                                                   \
    do {                                                                                                 \
        if (h == 0 && p_raw < n_points) {                                                                \
            const float inv = OUT_INV(L_);                                                               \
            const f32x4 o = {acc_[0][0] * inv + bias[(BIAS_) + 0], acc_[0][1] * inv + bias[(BIAS_) + 1], \
                             acc_[0][2] * inv + bias[(BIAS_) + 2], sigma_raw};                           \
            reinterpret_cast<f32x4*>(raw)[p_raw] = o;                                                    \
        }                                                                                                \
        NFB_RANGE_GUARD();                                                                               \
    } while (0)
