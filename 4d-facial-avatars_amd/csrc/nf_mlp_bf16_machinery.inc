// Table-driven machinery of the split-bf16 fused MLP kernels (weight-stream -> LDS ring, stage/layer drivers, operand split,
// activation saves).  Included by the forward (nf_mlp_*bf16_kernel.inc) and backward-chain (nf_mlp_*bf16_bwd.hip) kernels of both
// families after nf_mlp_split_common.h and the layer table namespace nfb { NL, KS[], NO[] } of THEIR weight stream with what
// nf_mlp_split_table.h derives from it.  The kernel text the families share: nf_mlp_split_fwd.inc, nf_mlp_split_bwd.inc.
// =================================================================================================
// forward
// =================================================================================================
// Weight stream -> LDS pipeline.  A stage = NFB_KPS k-steps of one layer (all of its output tiles, hi and lo):
// <= 32 KiB.  Three LDS buffers form a ring; the DMA of stage g+2 is issued while stage g is consumed, and the
// end-of-stage wait is a COUNTED s_waitcnt vmcnt(n) that leaves exactly that newest group in flight across the
// (raw) workgroup barrier.  Per-call biases are DMA'd once into LDS so that no ordinary global load (whose
// compiler-inserted vmcnt(0) would drain the pipeline) remains in the layer loop.  All LDS lives in ONE array.
#define NFB_KPS 2                                   // k-steps per stage
#define NFB_STAGE_BYTES (NFB_KPS * 8 * 2 * 1024)    // largest stage: 8 tiles x (hi, lo) x 1 KiB per k-step = 32 KiB
#define NFB_NBUF 4                                  // ring depth; stage g + NFB_NBUF - 1 is prefetched while stage g is consumed
#define NFB_STAGGER_DIV 4                           // wave w issues its DMA burst after w / DIV of the stage's MFMAs
#define NFB_LA (NFB_NBUF - 1)
#define NFB_BIAS_BLOCKS 10                          // cond table (2332 f32) padded to 10 KiB
#define NFB_XPOSE_PITCH 144                          // bytes per staged point row (128 + 16: conflict-free ds_write_b128)
#define NFB_XPOSE_BYTES (32 * NFB_XPOSE_PITCH)      // per wave: one [32 points][32 features] f32 tile on its way to HBM
#define NFB_XPOSE_OFF (NFB_NBUF * NFB_STAGE_BYTES + NFB_BIAS_BLOCKS * 1024)
#define NFB_LDS_BYTES (NFB_XPOSE_OFF + 4 * NFB_XPOSE_BYTES)

namespace nfb {
// global stage table (compile time): stage g -> (first stream block, number of blocks)
constexpr int stages_of(int l) { return KS[l] / NFB_KPS; }
constexpr int stage0_of(int l) { int o = 0; for (int i = 0; i < l; ++i) o += stages_of(i); return o; }
// NFB_RUN_LAYERS (density-only kernels): the kernel ends behind stream layer NFB_RUN_LAYERS - 1.  The ring then ends there too: a
// stage past it has no blocks, so it is never issued (stage_nblk) and never waited for (inflight_after), and the last stage that
// runs leaves with vmcnt(0) -- no DMA into LDS is outstanding at kernel exit.
#ifndef NFB_RUN_LAYERS
#define NFB_RUN_LAYERS NL
#endif
constexpr int N_STAGES = stage0_of(NFB_RUN_LAYERS);
constexpr int layer_of_stage(int g) { int l = 0; while (l < NL && g >= stage0_of(l + 1)) ++l; return l; }
constexpr int stage_nblk(int g) { return (g < 0 || g >= N_STAGES) ? 0 : 2 * NFB_KPS * NO[layer_of_stage(g)]; }
// DMA pieces of this wave that may stay in flight when stage g ends: those of stages g+2 .. g+NFB_LA
constexpr int inflight_after(int g) { int n = 0; for (int k = 2; k <= NFB_NBUF - 1; ++k) n += stage_nblk(g + k) / 4; return n; }
constexpr int stage_blk0(int g) {
    if (g < 0 || g >= N_STAGES) return 0;
    const int l = layer_of_stage(g);
    return 2 * pair_off(l) + (g - stage0_of(l)) * 2 * NFB_KPS * NO[l];
}
}  // namespace nfb

__host__ __device__ constexpr int64_t nfb_pad32(int64_t n) { return (n + 31) & ~(int64_t)31; }   // section length of the split training layouts

typedef __attribute__((address_space(3))) char nfb_lds_char;
struct NfbCtx {
    char* lds;               // workgroup LDS base
    nfb_lds_char* lds3;      // the same as an LDS-address-space pointer: the M0 value of a DMA piece is then ONE s_mov (a generic pointer costs a
                             // null check -- s_cmp_lg_u64 + s_cselect -- per piece: 2 x 484 scalar instructions per wave tile)
    int lane, wave;
    __amdgpu_buffer_rsrc_t wrsrc;   // the weight stream as a buffer: LDS-DMA pieces are addressed by ONE constant VGPR (lane * 16)
    unsigned wvoff;                 // ... plus a scalar block offset -- no 64-bit vector address arithmetic between the MFMAs
};
__device__ __forceinline__ void nfb_ctx_stream(NfbCtx& cx, const char* wstream, unsigned stream_bytes) {
    cx.wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(wstream), (short)0, (int)stream_bytes, 0x00020000);
    cx.wvoff = (unsigned)cx.lane * 16u;
    cx.lds3 = (nfb_lds_char*)cx.lds;
}

template <int N> __device__ __forceinline__ void nfb_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// LDS-DMA of NBLK 1-KiB blocks, stream block blk0.. -> LDS byte offset lds_off (block b is fetched by wave b % 4).
template <int NBLK>
__device__ __forceinline__ void nfb_issue(const NfbCtx& cx, const char* gsrc, int blk0, int lds_off) {
#pragma unroll
    for (int q = 0; q < (NBLK + 3) / 4; ++q) {
        const int b = cx.wave + 4 * q;
        if (NBLK % 4 == 0 || b < NBLK)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc + (size_t)(blk0 + b) * 1024),
                                             (__attribute__((address_space(3))) void*)(cx.lds3 + lds_off + b * 1024), 16, 0, 0);
    }
}

// weight-stream form of nfb_issue: buffer-descriptor LDS-DMA (buffer_load_dwordx4 ... lds), scalar block offsets
template <int NBLK>
__device__ __forceinline__ void nfb_issue_w(const NfbCtx& cx, int blk0, int lds_off) {
#pragma unroll
    for (int q = 0; q < (NBLK + 3) / 4; ++q) {
        const int b = cx.wave + 4 * q;
        if (NBLK % 4 == 0 || b < NBLK)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(cx.wrsrc, (__attribute__((address_space(3))) void*)(cx.lds3 + lds_off + b * 1024), 16,
                                                     (int)cx.wvoff, (blk0 + b) * 1024, 0, 0);
    }
}

// =================================================================================================
// deferred saves (training kernels): a layer's f32 output tiles leave for HBM from inside the NEXT layer's K loop
// =================================================================================================
// The training forward / backward chain keep TWO accumulator sets and alternate between them: while layer l+1 accumulates into one,
// the other still holds layer l's finished output (post-activation values / pre-activation gradients), and its [32 points][32
// features] tiles take a detour through a wave-private LDS slab one at a time (ds_write_b128 in register order, ds_read_b128 in row order; 144-byte row
// pitch: conflict-free; a store of 64 x 16 B straight from the registers would touch 64 lines with 16 bytes each), spread over the stages of layer l+1:
//     W(t): 4 ds_write_b128 (register order)   R(t): 4 ds_read_b128 (row order) into 16 transit registers   G(t): 4 stores
// a few MFMAs apart, so that no wait is exposed.  Rounds 1-3 issued all 32 store instructions of a layer (32 KiB per wave) in one
// burst at the layer boundary, with the matrix pipe idle (one in-order wave per SIMD) and every CU of the chip in the same
// phase: the kernels ran at (MFMA time + HBM write time) instead of max(...), and every stage-end vmcnt behind the burst also
// waited for the stores.  Stores are non-temporal and go through a buffer descriptor that covers exactly the section: rows past
// n_points are dropped by the range check (no predicate, no branch).  Counted stage waits: see nfb_stage.
struct NfbNoSide {
    static constexpr int stores_in_stage(int) { return 0; }
    __device__ __forceinline__ void at(int, int, int) {}
};

struct NfbSaveTarget {
    __amdgpu_buffer_rsrc_t rsrc;      // [n_points][width] row-major f32 section
    unsigned voff;                    // this lane's byte offset: row (p_tile + lane / 8), 16-byte chunk (lane % 8) of a tile's 128 bytes
};
__device__ __forceinline__ NfbSaveTarget nfb_save_target(float* sec, int width, int64_t p_tile, int64_t n_points, int lane) {
    NfbSaveTarget t;
    t.rsrc = __builtin_amdgcn_make_buffer_rsrc(sec, (short)0, (int)((unsigned)n_points * (unsigned)(4 * width)), 0x00020000);
    t.voff = ((unsigned)p_tile + (unsigned)(lane >> 3)) * (unsigned)(4 * width) + (unsigned)(lane & 7) * 16u;
    return t;
}
typedef unsigned nfb_u32x4 __attribute__((ext_vector_type(4)));
#define NFB_SAVE_AUX 2                                      // nt: the saves are read next by another kernel, from HBM
__device__ __forceinline__ void nfb_tile_to_slab(char* slab, const f32x16& a, int lane) {
    const int h = lane >> 5, c = lane & 31;
    *reinterpret_cast<f32x4*>(slab + c * NFB_XPOSE_PITCH + (0 + 4 * h) * 4) = (f32x4){a[0], a[1], a[2], a[3]};
    *reinterpret_cast<f32x4*>(slab + c * NFB_XPOSE_PITCH + (8 + 4 * h) * 4) = (f32x4){a[4], a[5], a[6], a[7]};
    *reinterpret_cast<f32x4*>(slab + c * NFB_XPOSE_PITCH + (16 + 4 * h) * 4) = (f32x4){a[8], a[9], a[10], a[11]};
    *reinterpret_cast<f32x4*>(slab + c * NFB_XPOSE_PITCH + (24 + 4 * h) * 4) = (f32x4){a[12], a[13], a[14], a[15]};
}
__device__ __forceinline__ void nfb_slab_to_transit(const char* slab, f32x4 (&tr)[4], int lane) {
    const int pt = lane >> 3, ch = lane & 7;
#pragma unroll
    for (int k = 0; k < 4; ++k) tr[k] = *reinterpret_cast<const f32x4*>(slab + (8 * k + pt) * NFB_XPOSE_PITCH + ch * 16);
}
template <int WIDTH>
__device__ __forceinline__ void nfb_transit_to_global(const f32x4 (&tr)[4], const NfbSaveTarget& tg, int nt) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(nfb_u32x4, tr[k]), tg.rsrc, (int)tg.voff, 8 * k * (4 * WIDTH) + 128 * nt,
                                               NFB_SAVE_AUX);
}

// NOP tiles (WIDTH = 32 NOP floats per point) of the PREVIOUS layer's output, saved from inside the NST stages of this layer
template <int NOP, int NST>
struct NfbSaveSide {
    const f32x16 (&sv)[8];
    NfbSaveTarget tg;
    char* slab;
    int lane;
    f32x4 tr[4];
    static constexpr int TPS = (NOP + NST - 1) / NST;                 // tiles per stage
    static constexpr int first_tile(int i) { return i * TPS < NOP ? i * TPS : NOP; }
    static constexpr int tiles_in_stage(int i) { return (i < 0 || i >= NST) ? 0 : first_tile(i + 1) - first_tile(i); }
    static constexpr int stores_in_stage(int i) { return 4 * tiles_in_stage(i); }
    __device__ __forceinline__ NfbSaveSide(const f32x16 (&sv_)[8], const NfbSaveTarget& tg_, char* slab_, int lane_)
        : sv(sv_), tg(tg_), slab(slab_), lane(lane_) {}
    // called before MFMA number m (0 .. NM - 1) of stage i of the layer; everything folds after unrolling
    __device__ __forceinline__ void at(int i, int m, int NM) {
        const int k = tiles_in_stage(i);
        if (k == 0) return;
        const int region = NM / k, j = m / region;
        if (j >= k) return;
        const int r = m - j * region, d = region >= 3 ? region / 3 : 1, t = first_tile(i) + j;
        if (r == 0) {
            __builtin_amdgcn_sched_barrier(0);
            nfb_tile_to_slab(slab, sv[t], lane);
            __builtin_amdgcn_sched_barrier(0);
        } else if (r == d) {
            __builtin_amdgcn_sched_barrier(0);
            nfb_slab_to_transit(slab, tr, lane);
            __builtin_amdgcn_sched_barrier(0);
        } else if (r == 2 * d) {
            __builtin_amdgcn_sched_barrier(0);
            nfb_transit_to_global<32 * NOP>(tr, tg, t);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
};
// the whole output at once (the last layer of a kernel has no K loop behind it): same path, back to back
template <int NOP>
__device__ __forceinline__ void nfb_save_now(const f32x16 (&sv)[8], const NfbSaveTarget& tg, char* slab, int lane) {
#pragma unroll
    for (int t = 0; t < NOP; ++t) {
        f32x4 tr[4];
        nfb_tile_to_slab(slab, sv[t], lane);
        __builtin_amdgcn_wave_barrier();
        nfb_slab_to_transit(slab, tr, lane);
        nfb_transit_to_global<32 * NOP>(tr, tg, t);
        __builtin_amdgcn_wave_barrier();
    }
}

// =================================================================================================
// training FORWARD: saved activations leave as the weight-gradient kernel's operand fragments
// =================================================================================================
// What the forward keeps for the backward is read by ONE consumer, the split weight-gradient GEMM dW = dZ^T . X, whose K dimension
// is the point: its MFMA operand wants "lane = feature, 8 K-slots = 8 points" as (hi, lo) 16-bit pairs -- the transpose of what
// this kernel holds (lane = point, 8 K-slots = 8 features), and exactly the (hi, lo) split it has ALREADY computed for its own next
// layer.  Rounds 1-4a wrote f32 rows (an LDS transpose per tile here: +25 % LDS traffic on an LDS-bound kernel) and the dW kernel
// re-read them with eight strided dword loads per lane and split them again.  Now the matrix core does the transpose:
//     D[point][feature] = X_hi[point][k] . SEL[k][feature]          (SEL = 0/1 selection matrix; exact: one product per output)
// i.e. v_mfma with the layer's operand registers (bh / bl, alive anyway during the next layer's K loop) as the A operand.  D holds
// lane = feature, registers = 16 + 16 points; two packed converts per 4 registers give the dW kernel's fragment, stored lane-linearly
// (1 KiB per instruction).  Per [32 points][32 features] tile: 4 MFMAs (+8 % of a layer's), 16 converts, 4 stores -- no LDS, no
// second accumulator set; the dW kernel DMAs the blocks straight into its LDS ring (no conversion, no strided loads).
// Stream layout of a section of NO tiles (32 NO features per point), n_pad = points rounded up to 32:
//     block ((p / 16) NO + tile) 2 + (0: hi, 1: lo)  =  1 KiB = [lane (h, c)][8 x 16 bit]:  feature 32 tile + c,
//     K-slot j of lane half h  <->  point 16 (p / 16) + 4 h + (j & 3) + 8 (j >> 2)                      (nfb_dw_point_of_slot)
// (fp16 instantiation: values x 2^NFB_ACT_SHIFT, as the operands carry them and as the fp16 dW kernel scales saved activations.)
__device__ __forceinline__ void nfb_sel_operands(bf16x8 (&sel)[2], int lane) {
    const int h = lane >> 5, c = lane & 31;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) sel[u][j] = (nfb_elt)((c == 16 * u + 4 * h + (j & 3) + 8 * (j >> 2)) ? 1.0f : 0.0f);
}
struct NfbStreamTarget {
    __amdgpu_buffer_rsrc_t rsrc;      // the section's fragment stream
    unsigned voff;                    // this wave's first block pair + lane * 16
};
__device__ __forceinline__ NfbStreamTarget nfb_stream_target(float* sec, int n_tiles, int64_t p_tile, int64_t n_pad, int lane) {
    NfbStreamTarget t;
    t.rsrc = __builtin_amdgcn_make_buffer_rsrc(sec, (short)0, (int)((unsigned)n_pad * (unsigned)(128 * n_tiles)), 0x00020000);
    t.voff = (unsigned)(p_tile >> 4) * (unsigned)(2048 * n_tiles) + (unsigned)lane * 16u;
    return t;
}
// NOP tiles of the previous layer's output = operand k-steps OFF .. OFF + 2 NOP - 1 of (oh, ol), streamed from inside the NST stages
template <int NOP, int NST, int OFF>
struct NfbStreamSide {
    const bf16x8 (&oh)[20];
    const bf16x8 (&ol)[20];
    const bf16x8 (&sel)[2];
    NfbStreamTarget tg;
    f32x16 dh;
    static constexpr int TPS = (NOP + NST - 1) / NST;                 // tiles per stage
    static constexpr int first_tile(int i) { return i * TPS < NOP ? i * TPS : NOP; }
    static constexpr int tiles_in_stage(int i) { return (i < 0 || i >= NST) ? 0 : first_tile(i + 1) - first_tile(i); }
    static constexpr int stores_in_stage(int i) { return 4 * tiles_in_stage(i); }
    __device__ __forceinline__ NfbStreamSide(const bf16x8 (&oh_)[20], const bf16x8 (&ol_)[20], const bf16x8 (&sel_)[2], const NfbStreamTarget& tg_)
        : oh(oh_), ol(ol_), sel(sel_), tg(tg_) {}
    // (hi and lo take turns in ONE set of 16 result registers: the fp16 instantiations have none to spare)
    // the two products of a tile half depend on each other through D: they sit in consecutive MFMA slots of the main loop (an
    // independent MFMA of the layer between them), not back to back
    __device__ __forceinline__ void xpose(const bf16x8 (&o)[20], int t, int part) {
        __builtin_amdgcn_sched_barrier(0);
        if (part == 0) {
            f32x16 z;
#pragma unroll
            for (int q = 0; q < 16; ++q) z[q] = 0.0f;
            dh = NFB_MFMA(o[OFF + 2 * t], sel[0], z, 0, 0, 0);
        } else {
            dh = NFB_MFMA(o[OFF + 2 * t + 1], sel[1], dh, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void flush(int t, int hl) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            bf16x8 f;
#pragma unroll
            for (int q = 0; q < 8; ++q) f[q] = (nfb_elt)dh[8 * u + q];                                  // exact: D holds 16-bit values
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(nfb_u32x4, f), tg.rsrc, (int)tg.voff, ((u * NOP + t) * 2 + hl) * 1024, NFB_SAVE_AUX);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void at(int i, int m, int NM) {
        const int k = tiles_in_stage(i);
        if (k == 0) return;
        const int region = NM / k, j = m / region;
        if (j >= k) return;
        const int r = m - j * region, d = region >= 6 ? region / 3 : 2, t = first_tile(i) + j;      // (region >= 6: every layer's stages)
        if (r == 0) xpose(oh, t, 0);                        // results are consumed d MFMAs later
        else if (r == 1) xpose(oh, t, 1);
        else if (r == d) { flush(t, 0); xpose(ol, t, 0); }
        else if (r == d + 1) xpose(ol, t, 1);
        else if (r == 2 * d) flush(t, 1);
    }
};
#define NFB_LAYER_STREAMING(L_, acc_, bh_, bl_, NOP_, oh_, ol_, sel_, tg_)                                              \
    do {                                                                                                                \
        typedef NfbStreamSide<NOP_, nfb::stages_of(L_), 4> side_t_;                                                     \
        side_t_ side_(oh_, ol_, sel_, tg_);                                                                             \
        nfb_layer<nfb::stage0_of(L_), nfb::stages_of(L_), nfb::NO[L_], 0, side_t_>(cx, acc_, bh_, bl_, side_);         \
    } while (0)

// Stage G (compile time): consume stage G out of ring buffer G % 3 while prefetching stage G+2, then leave only that
// newest DMA group in flight (counted vmcnt) and cross the workgroup barrier.
// The four waves issue their DMA bursts at DIFFERENT points of the stage (wave w after a quarter w of its MFMAs): the
// CU has one texture-address unit, and four simultaneous bursts right behind the barrier make every wave wait for all
// 4 x NQ pieces to be accepted; staggered, a wave only waits for its own.
// SIDE (NfbNoSide / NfbSaveSide): memory work of the training kernels interleaved with the MFMAs of the stage; I = index of the stage
// within its layer.  vmcnt retires in order and counts stores too: the stage-end wait allows the DMA pieces of the later stages AND
// the stores of this and the previous stage (all issued after the DMA group being waited for) to stay in flight.
// PM: which of the three products of the split are issued (bit 0: W_lo x_hi, bit 1: W_hi x_lo, bit 2: W_hi x_hi).  7 = the split
// arithmetics proper ("x3"); 5 = "f16x2" (nf_mlp_f16x2.hip): activations enter with their 11-bit fp16 `hi` part only, the weights keep
// their 22 bits -- a third fewer MFMAs; which term can go was measured per layer in profiles/r05_split_products.md.
template <int G, int NO, int I = 0, class SIDE = NfbNoSide, int PM = 7>
__device__ __forceinline__ void nfb_stage(const NfbCtx& cx, f32x16 (&acc)[8], const bf16x8 (&bh)[20], const bf16x8 (&bl)[20], int s0, SIDE& side) {
    constexpr int nb2 = nfb::stage_nblk(G + NFB_LA);
    constexpr int blk2 = nfb::stage_blk0(G + NFB_LA);
    constexpr int off2 = ((G + NFB_LA) % NFB_NBUF) * NFB_STAGE_BYTES;
    constexpr int NM = NFB_KPS * ((PM & 1) + ((PM >> 1) & 1) + ((PM >> 2) & 1)) * NO;     // MFMAs in this stage
    const char* base = cx.lds + (G % NFB_NBUF) * NFB_STAGE_BYTES + cx.lane * 16;
    int m = 0;                                                // MFMA counter (compile time after unrolling)
#ifndef NFB_TILE_GROUP
#define NFB_TILE_GROUP 8                                      // output tiles whose A fragments are held in registers at once
#endif
    constexpr int TG = NO < NFB_TILE_GROUP ? NO : NFB_TILE_GROUP;
#pragma unroll
    for (int u = 0; u < NFB_KPS; ++u) {
#pragma unroll
        for (int n0 = 0; n0 < NO; n0 += TG) {
            bf16x8 ah[TG], al[TG];
#pragma unroll
            for (int nt = 0; nt < TG; ++nt) {
                ah[nt] = *reinterpret_cast<const bf16x8*>(base + ((u * NO + n0 + nt) * 2 + 0) * 1024);
                al[nt] = *reinterpret_cast<const bf16x8*>(base + ((u * NO + n0 + nt) * 2 + 1) * 1024);
            }
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int nt = 0; nt < TG; ++nt) {
                    if (!((PM >> t) & 1)) continue;
                    if (nb2 > 0) {
#pragma unroll
                        for (int w = 0; w < 4; ++w)
                            if (m == (w * NM) / NFB_STAGGER_DIV && cx.wave == w)
                                nfb_issue_w<(nb2 > 0 ? nb2 : 4)>(cx, blk2, off2);
                    }
                    side.at(I, m, NM);
                    const bf16x8& a = t == 0 ? al[nt] : ah[nt];
                    const bf16x8& b = t == 1 ? bl[s0 + u] : bh[s0 + u];
                    acc[n0 + nt] = NFB_MFMA(a, b, acc[n0 + nt], 0, 0, 0);
                    ++m;
                }
        }
    }
    nfb_wait_vm<nfb::inflight_after(G) + SIDE::stores_in_stage(I) + SIDE::stores_in_stage(I - 1)>();   // stage G+1 has landed for this wave; later stages may still fly
    __builtin_amdgcn_s_barrier();                             // ... and for every wave; buffer G % 3 is free again
    asm volatile("" ::: "memory");
}

template <int G0, int NST, int NO, int I = 0, class SIDE = NfbNoSide, int PM = 7>
__device__ __forceinline__ void nfb_layer(const NfbCtx& cx, f32x16 (&acc)[8], const bf16x8 (&bh)[20], const bf16x8 (&bl)[20], SIDE& side) {
    if constexpr (I < NST) {
        nfb_stage<G0 + I, NO, I, SIDE, PM>(cx, acc, bh, bl, NFB_KPS * I, side);
        nfb_layer<G0, NST, NO, I + 1, SIDE, PM>(cx, acc, bh, bl, side);
    }
}
#ifndef NFB_PRODUCTS
#define NFB_PRODUCTS 7                                        // set by the translation unit of an arithmetic (nf_mlp_f16x2.hip: 5)
#endif
#define NFB_LAYER(L_, acc_, bh_, bl_)                                                                                   \
    do { NfbNoSide no_side_; nfb_layer<nfb::stage0_of(L_), nfb::stages_of(L_), nfb::NO[L_], 0, NfbNoSide, NFB_PRODUCTS>(cx, acc_, bh_, bl_, no_side_); } while (0)
// layer L_ accumulating into acc_ while the NOP_ tiles of sv_ (the previous layer's output) leave for section target tg_
#define NFB_LAYER_SAVING(L_, acc_, bh_, bl_, NOP_, sv_, tg_)                                                            \
    do {                                                                                                                \
        NfbSaveSide<NOP_, nfb::stages_of(L_)> side_(sv_, tg_, cx.lds + NFB_XPOSE_OFF + cx.wave * NFB_XPOSE_BYTES, cx.lane); \
        nfb_layer<nfb::stage0_of(L_), nfb::stages_of(L_), nfb::NO[L_], 0, NfbSaveSide<NOP_, nfb::stages_of(L_)>>(cx, acc_, bh_, bl_, side_); \
    } while (0)

__device__ __forceinline__ void nfb_split(const float (&x)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const nfb_elt h = (nfb_elt)x[j];
        hi[j] = h;
        lo[j] = (nfb_elt)(x[j] - (float)h);
    }
}

// accumulators (NO tiles) -> B operands of the next layer: tile nt, regs 8u..8u+7 -> k-step 2 nt + u
// `inv` un-does the layer's weight scale (fp16 instantiation; exactly 1 and folded away for bf16).
template <int NO, bool RELU>
__device__ __forceinline__ void nfb_to_operands(const f32x16 (&acc)[8], bf16x8 (&bh)[20], bf16x8 (&bl)[20], int s_off, float inv = 1.0f) {
#pragma unroll
    for (int nt = 0; nt < NO; ++nt)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = acc[nt][8 * u + j] * inv;
                x[j] = RELU ? __builtin_amdgcn_fmed3f(v, 0.f, __builtin_inff()) : v;
            }
            nfb_split(x, bh[s_off + 2 * nt + u], bl[s_off + 2 * nt + u]);
        }
}

#if NFB_F16
// fp16 forward kernels (round 6): the same values with half the vector instructions.  The layer scale `inv` is a power of two, so
//     med3(acc * inv, 0, 65504) = med3(acc, 0, sat_raw) * inv                     (sat_raw = 65504 / inv, exact),
// the ReLU runs on the RAW accumulator and the scale rides inside the conversions as the multiplier of v_fma_mixlo/mixhi_f16
// (f32 sources, f16 result written to one half of the packed register):
//     hi = f16(fma(r, inv, 0))          lo = f16(fma(r, inv, -hi))                (r * inv is exact; r * inv - hi is exact in f32)
// -- 3 instructions per element (med3, 2 mix) instead of mul + med3 + cvt_pk / 2 + cvt_f32_f16 + sub + cvt_pk / 2 = 5, bit for bit.
template <int NO, bool RELU>
__device__ __forceinline__ void nfb_to_operands_f16(const f32x16 (&acc)[8], bf16x8 (&bh)[20], bf16x8 (&bl)[20], int s_off, float inv, float sat_raw) {
#pragma unroll
    for (int nt = 0; nt < NO; ++nt)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            bf16x8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float r = acc[nt][8 * u + j];
                if (RELU) r = __builtin_amdgcn_fmed3f(r, 0.f, sat_raw);
                const _Float16 h = (_Float16)__builtin_fmaf(r, inv, 0.0f);
                hi[j] = h;
                lo[j] = (_Float16)__builtin_fmaf(r, inv, -(float)h);
            }
            bh[s_off + 2 * nt + u] = hi;
            bl[s_off + 2 * nt + u] = lo;
        }
}
#endif

// ReLU bit mask of a layer output (training forward): bit 16 nt + r of this lane half <-> acc[nt][r] > 0
__host__ __device__ constexpr int nfb_mask_index(int sec) {
    return sec == nfl::S_H0 ? 0 : sec == nfl::S_H1 ? 1 : sec == nfl::S_H2 ? 2 : sec == nfl::S_H3 ? 3 : sec == nfl::S_H4 ? 4 :
           sec == nfl::S_H5 ? 5 : sec == nfl::S_D0 ? 6 : sec == nfl::S_D1 ? 7 : sec == nfl::S_D2 ? 8 : -1;
}
template <int NO>
__device__ __forceinline__ void nfb_save_mask(const f32x16 (&acc)[8], float* __restrict__ mask_sec, int layer, int64_t n_points, int64_t p,
                                              int h) {
    // bit = [x > 0] = sign bit of -(int)bits(x) for every x but -0.0 (whose product with its mask bit is 0 either way); each bit is
    // funnel-shifted into its word from the right, highest position first: 2 instructions per accumulator register
    unsigned m[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int w = 0; w < (NO + 1) / 2; ++w)
#pragma unroll
        for (int k = 31; k >= 0; --k) {
            const int nt = 2 * w + (k >> 4), r = k & 15;
            const unsigned neg = nt < NO ? 0u - __float_as_uint(acc[nt][r]) : 0u;
            m[w] = __builtin_amdgcn_alignbit(m[w], neg, 31);           // (m << 1) | (neg >> 31)
        }
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    reinterpret_cast<u32x4_t*>(mask_sec)[((int64_t)layer * n_points + p) * 2 + h] = (u32x4_t){m[0], m[1], m[2], m[3]};
}

#if NFB_F16
// ---- block floating point of the fp16 backward chain ------------------------------------------------------------------------
// A lane of the 32 x 32 accumulator tiles holds features of ONE point (lanes c and c + 32 share point c), and a column of the
// B operand scales its output column linearly, so every point carries its own power-of-two gradient scale g: after each layer
// the true gradients (accumulator / (s_W g)) are written to dz, the point's largest |gradient| picks the next g so that the
// operands sit in [2^13, 2^14) at the top of fp16's range -- the (hi, lo) pair then holds 22 bits of every gradient down to
// 2^-19 of the point's largest one, where a per-launch scale left hidden-layer gradients in fp16's subnormals.
// The weight-gradient kernel needs ONE scale per dz section (its K dimension runs over points): the chain leaves max |dz| of
// every section in `lmax` (float bits, zero on entry): per-lane maxima ride along in registers, one reduction per wave at the end.
#define NFB_GS_DRAW 10                                   // slot of max |d_raw|; slots 0..9: the chain's layers in kernel order
template <int NO>
__device__ __forceinline__ float nfb_lane_absmax(const f32x16 (&acc)[8]) {
    float m = 0.0f;
#pragma unroll
    for (int nt = 0; nt < NO; ++nt)
#pragma unroll
        for (int r = 0; r < 16; r += 2) m = fmaxf(m, fmaxf(fabsf(acc[nt][r]), fabsf(acc[nt][r + 1])));
    return m;
}
// g = 2^(13 - k) for m in [2^k, 2^(k+1)) (m >= 0; zero, denormal, huge and non-finite m clamp to exponents in [-60, 60])
__device__ __forceinline__ float nfb_pow2_scale(float m, float& inv) {
    const int e = (int)(__float_as_uint(m) >> 23);                    // biased exponent (sign bit clear)
    int se = 267 - e;                                                 // 127 + 13 - (e - 127)
    se = se < 67 ? 67 : (se > 187 ? 187 : se);
    inv = __uint_as_float((unsigned)(254 - se) << 23);
    return __uint_as_float((unsigned)se << 23);
}
// the point's max from the lane's: lanes c and c + 32 hold the two halves of point c's features (one VALU swap, no LDS)
__device__ __forceinline__ float nfb_pair_max(float m) {
    const unsigned b = __float_as_uint(m);
    const auto r = __builtin_amdgcn_permlane32_swap(b, b, false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
// end of the kernel: lm[i] = this lane's max of section i; the wave's maxima go to lmax[0..N) -- N independent butterfly
// reductions issued together (their latencies overlap), then ONE atomicMax instruction from lanes 0..N-1, and only where the
// wave beats the (possibly stale) value it saw at the start of the kernel
template <int N>
__device__ __forceinline__ void nfb_flush_layer_max(const float (&lm)[N], unsigned* __restrict__ lmax, unsigned seen, int lane) {
    float w[N];
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = lm[i];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < N; ++i) w[i] = fmaxf(w[i], __shfl_xor(w[i], o, 64));
    float mine = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) mine = lane == i ? w[i] : mine;
    const unsigned mb = __float_as_uint(mine);
    if (lane < N && mb > seen && mb < 0x7f800000u) atomicMax(lmax + lane, mb);
}
#endif

// backward chain: d sigma joins the operands (th, tl) as k-step S, slot (0, 0) of the lanes that are `on`, at the scale g of the
// k-steps in front of it; k-step S + 1 is zero
template <int S>
__device__ __forceinline__ void nfb_dsigma_kstep(bf16x8 (&th)[20], bf16x8 (&tl)[20], bool on, float d_sigma, float g) {
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (on) x[0] = d_sigma * g;
    nfb_split(x, th[S], tl[S]);
#pragma unroll
    for (int j = 0; j < 8; ++j) { th[S + 1][j] = (nfb_elt)0.f; tl[S + 1][j] = (nfb_elt)0.f; }
}

template <int NO>
__device__ __forceinline__ void nfb_scale(f32x16 (&acc)[8], float s) {
#pragma unroll
    for (int nt = 0; nt < NO; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] *= s;
}

// acc[nt] reg r <- bias[32 nt + (r&3) + 8 (r>>2) + 4 h]   (bias table in LDS)
template <int NO>
__device__ __forceinline__ void nfb_init_bias(f32x16 (&acc)[8], const float* bias, int h) {
#pragma unroll
    for (int nt = 0; nt < NO; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(bias + 32 * nt + 8 * q + 4 * h);
            acc[nt][4 * q + 0] = b.x; acc[nt][4 * q + 1] = b.y; acc[nt][4 * q + 2] = b.z; acc[nt][4 * q + 3] = b.w;
        }
}

__device__ __forceinline__ void nfb_zero(f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

template <int NO>
__device__ __forceinline__ void nfb_zero_tiles(f32x16 (&acc)[8]) {
#pragma unroll
    for (int nt = 0; nt < NO; ++nt) nfb_zero(acc[nt]);
}

// backward chain: acc[nt] reg r keeps its value where bit (16 nt + r) of the lane's 128-bit ReLU mask (nfb_save_mask) is set
template <int NO>
__device__ __forceinline__ void nfb_apply_mask(f32x16 (&acc)[8], const nfb_u32x4& m) {
#pragma unroll
    for (int nt = 0; nt < NO; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned bit = (m[nt >> 1] >> (16 * (nt & 1) + r)) & 1u;
            acc[nt][r] = bit ? acc[nt][r] : 0.0f;
        }
}

