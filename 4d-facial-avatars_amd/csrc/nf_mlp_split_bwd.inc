// The family-independent text of the split-precision backward chain dZ_l = (dZ_{l+1} . W_{l+1}) * [X_l > 0], included ONCE, as the
// first statements of the body of a family's __global__ chain kernel (nf_mlp_bf16_bwd.hip: paper model; nf_mlp_lcode_bf16_bwd.hip:
// second family).  Text and not a function for the reason given in nf_mlp_split_fwd.inc.  The kernel's parameters are the names
// used here (wstream, saved, d_raw, n_points, dz, gscale).  The family provides, before the #include:
//   NfbChain                   S_MASK: the section of `saved` that holds the ReLU bit masks; N_MASKS: how many the chain reads
// What stands behind this file in the kernel body: the family's layer list, written with the macros defined at the end of this
// file and nfb_dsigma_kstep (machinery); its last line is NFB_BWD_LAST.
//
// ---- front: tile, scales, d_raw and the masks, ring start, the rgb-gradient k-step -------------------------------------------
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
    const bool live = p_raw < n_points;
    const int64_t n = n_points;
    // The 16-bit-input MFMA accumulates with a small rounding bias toward -inf (about -2^-26 of the addends, measured: profiles/
    // r02_experiments.md section 8) that survives in sums over points where the gradients themselves cancel (bias gradients:
    // sum |dz| / |sum dz| = 300 ... 12000).  Every point therefore runs the chain with its own sign: odd points carry -gradient
    // in the operands (the sign is taken back when dz is written), so the bias alternates over points and cancels like noise.
    const float sgn = (c & 1) ? -1.0f : 1.0f;
#if NFB_F16
    // operands carry gradient * g, g the point's own (signed) power-of-two scale (block floating point, machinery.inc);
    // INV(l) = 1 / s_W(l), so INV(l) / g turns an accumulator into the true pre-activation gradient that is written to `dz`.
    // (the scales are pinned in SGPRs for the reason given in nf_mlp_split_fwd.inc)
    const float* __restrict__ wscale = reinterpret_cast<const float*>(wstream + (size_t)nfb::STREAM_BF16 * 2);
    float wsc[nfb::NL];
#pragma unroll
    for (int i = 0; i < nfb::NL; ++i) wsc[i] = wscale[nfb::NL + i];
#pragma unroll
    for (int i = 0; i < nfb::NL; ++i) asm volatile("" : "+s"(wsc[i]));
    unsigned* lmax = reinterpret_cast<unsigned*>(gscale);
    const unsigned seen = cx.lane < 16 ? __atomic_load_n(lmax + cx.lane, __ATOMIC_RELAXED) : 0u;   // possibly stale: only saves atomics
#define INV(L_) wsc[L_]
#else
    const float G = sgn, invG = sgn;
#define INV(L_) 1.0f
#endif

    // ordinary loads first (d_raw, the ReLU bit masks), then the ring
    const f32x4 d = reinterpret_cast<const f32x4*>(d_raw)[p];
    nfb_u32x4 mask[NfbChain::N_MASKS];
    const nfb_u32x4* mbase = reinterpret_cast<const nfb_u32x4*>(saved + (int64_t)NfbChain::S_MASK * nfb_pad32(n));   // (split training layout: sections are n rounded up to 32 points long)
#pragma unroll
    for (int l = 0; l < NfbChain::N_MASKS; ++l) mask[l] = mbase[((int64_t)l * n + p) * 2 + h];
    nfb_issue_w<nfb::stage_nblk(0)>(cx, nfb::stage_blk0(0), 0);
    nfb_issue_w<nfb::stage_nblk(1)>(cx, nfb::stage_blk0(1), NFB_STAGE_BYTES);
    nfb_issue_w<nfb::stage_nblk(2)>(cx, nfb::stage_blk0(2), 2 * NFB_STAGE_BYTES);

    bf16x8 bh[20], bl[20], th[20], tl[20];
#if NFB_F16
    // per-point gradient scales (block floating point, nf_mlp_bf16_machinery.inc)
    float invG;
    float lm[NFB_GS_DRAW + 1];                                          // this lane's max |gradient| per section (slots: machinery.inc)
#pragma unroll
    for (int i = 0; i <= NFB_GS_DRAW; ++i) lm[i] = 0.0f;
    lm[NFB_GS_DRAW] = live ? fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fmaxf(fabsf(d.z), fabsf(d.w))) : 0.0f;
    float G = sgn * nfb_pow2_scale(fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z)), invG);  // the rgb gradient of this point
    invG *= sgn;
#endif
    {
        float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (h == 0 && live) { x[0] = d.x * G; x[1] = d.y * G; x[2] = d.z * G; }
        nfb_split(x, th[0], tl[0]);
#pragma unroll
        for (int j = 0; j < 8; ++j) { th[1][j] = (nfb_elt)0.f; tl[1][j] = (nfb_elt)0.f; }
    }
    nfb_wait_vm<nfb::inflight_after(-1)>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    // two accumulator sets (deferred saves, nf_mlp_bf16_machinery.inc): dZ of layer l leaves from inside the K loop of layer l+1
    f32x16 accA[8], accB[8];

// ---- the layer macros of a family's layer list ------------------------------------------------------------------------------------
// EXTRA_: a gradient that joins the next layer's operands (d sigma), so that the point's scale covers it
#if NFB_F16
#define NFB_BWD_RESCALE(L_, acc_, NO_, EXTRA_)                                                           \
    do {                                                                                                 \
        lm[L_] = nfb_pair_max(live ? nfb_lane_absmax<NO_>(acc_) : 0.0f);                                 \
        G = sgn * nfb_pow2_scale(fmaxf(lm[L_], EXTRA_), invG);                                           \
        invG *= sgn;                                                                                     \
    } while (0)
#else
#define NFB_BWD_RESCALE(L_, acc_, NO_, EXTRA_) (void)0
#endif
// layer epilogue: ReLU mask number MASK_ (-1: no activation), true gradients (they stay in acc_ until the NEXT layer's K loop has
// stored them), next operands
#define NFB_BWD_FINISH(L_, acc_, NO_, MASK_, EXTRA_)                                                     \
    do {                                                                                                 \
        if ((MASK_) >= 0) nfb_apply_mask<NO_>(acc_, mask[(MASK_) >= 0 ? (MASK_) : 0]);                   \
        nfb_scale<NO_>(acc_, INV(L_) * invG);                      /* true gradients for dz */            \
        NFB_BWD_RESCALE(L_, acc_, NO_, EXTRA_);                                                          \
        nfb_to_operands<NO_, false>(acc_, bh, bl, 0, G);                                                 \
    } while (0)
// layer L_ into acc_ while the NOP_ tiles of prev_ (the layer before) leave for section PZSEC_ of dz
#define NFB_BWD_RUN(L_, acc_, oh_, ol_, NOP_, prev_, PZSEC_)                                             \
    do {                                                                                                 \
        const NfbSaveTarget tg_ = nfb_save_target(dz + (int64_t)(PZSEC_) * n, 32 * (NOP_), p_tile, n, cx.lane); \
        NFB_LAYER_SAVING(L_, acc_, oh_, ol_, NOP_, prev_, tg_);                                          \
    } while (0)
// the chain's last layer L_ (256 wide, finished in acc_): its dZ goes to section ZSEC_ at once -- it has no K loop behind it
#define NFB_BWD_LAST(L_, acc_, MASK_, ZSEC_)                                                             \
    do {                                                                                                 \
        if ((MASK_) >= 0) nfb_apply_mask<8>(acc_, mask[(MASK_) >= 0 ? (MASK_) : 0]);                     \
        nfb_scale<8>(acc_, INV(L_) * invG);                                                              \
        nfb_save_now<8>(acc_, nfb_save_target(dz + (int64_t)(ZSEC_) * n, 256, p_tile, n, cx.lane),       \
                        cx.lds + NFB_XPOSE_OFF + cx.wave * NFB_XPOSE_BYTES, cx.lane);                    \
        NFB_BWD_RESCALE(L_, acc_, 8, 0.0f);          /* only for max |dZ| of the section (the weight-gradient kernel's scale) */ \
        NFB_BWD_FLUSH_MAX();                                                                             \
    } while (0)
#if NFB_F16
#define NFB_BWD_FLUSH_MAX() nfb_flush_layer_max<NFB_GS_DRAW + 1>(lm, lmax, seen, cx.lane)
#else
#define NFB_BWD_FLUSH_MAX() (void)0
#endif
