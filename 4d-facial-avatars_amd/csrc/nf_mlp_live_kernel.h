// k_paper_mlp_fwd_live and what launches it: the kernel of nf_mlp_live.hip (the description stands there), written once for its two
// instantiations -- the production kernel (nf_mlp_live.hip) and the one that also counts what each wave did (nf_mlp_live_stats.hip) --
// and for k_paper_mlp_fwd_live<., ., GATE> (GATE; nf_mlp_gated.hip, nf_mlp_gated_stats.hip: the description stands there), the same schedule
// with "not proven dead" in place of "live" and fc_feat moved into the gathered run.
#pragma once
#include <mutex>
#include "nf_mlp_paper_net.h"

#define NF_LIVE_ROWS 64                                   // ring rows per wave (at most 31 are in use at a time)
#ifndef NF_LIVE_PF                                        // (a build flag for measuring other depths: profiles/live_colour_fill.md)
#define NF_LIVE_PF 8                                      // ring rows requested while fc_alpha's row runs
#endif
#define NF_LIVE_DIR_B (NF_LIVE_ROWS * 1024)               // byte offsets inside a wave's ring: [rows][64] feat fragments, then
#define NF_LIVE_META_B (NF_LIVE_DIR_B + NF_LIVE_ROWS * 64)     // [rows][4] direction fragments, then [rows] (index lo, hi, sigma_raw, -)
#define NF_LIVE_WAVE_B (NF_LIVE_META_B + NF_LIVE_ROWS * 16)
#define NF_LIVE_OOB NF_LIVE_WAVE_B                        // an offset the descriptor's range check drops (loads return 0)
#define NF_LIVE_SC1 16                                    // cache policy bit of the buffer loads: sc1

static_assert(NF_LIVE_ROWS == 64 && NF_MLP_NT == 2, "row numbers wrap with & 63; a pass's liveness is one 32-bit mask");
static_assert(NF_LIVE_PF >= 0 && NF_LIVE_PF <= 16, "prefetched rows live in registers beside fc_alpha's weights");

// the wave's ring as a buffer descriptor; the base comes back from its VGPR pair as a scalar (a descriptor in vector registers would put
// a waterfall loop around every access)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t nf_live_ring(char* ring_v) {
    const uint64_t a = (uint64_t)ring_v;
    const uint64_t s = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a) |
                       ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(s), (short)0, NF_LIVE_WAVE_B, 0x00020000);
}
__device__ __forceinline__ void nf_live_store(__amdgpu_buffer_rsrc_t ring, int off_b, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(nf_u32x4, v), ring, off_b, 0, 0);
}
__device__ __forceinline__ f32x4 nf_live_load(__amdgpu_buffer_rsrc_t ring, int off_b) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ring, off_b, 0, NF_LIVE_SC1));
}
// lowest set bit of a wave-uniform mask, taken off it
__device__ __forceinline__ int nf_live_pop(unsigned& m) {
    const int r = __builtin_ctz(m);
    m &= m - 1u;
    return r;
}
// slab address of fragment `lane` of row `prow` as the ring stores it (fragment = feature / 4)
__device__ __forceinline__ int nf_live_slab(int prow, int lane) { return nf_act_idx4(prow, lane); }

// What a pass requests while fc_alpha's row runs alone (the hook of nf_paper_net_body<..., SIGMA>): layers_dir.0's bias, first weight
// chunk and direction-chunk weights as a colour run finds them, and the oldest ring rows, lane l holding fragment l.  The ring's
// state comes from its VGPR homes and goes back to scalars here: nothing scalar crosses the trunk.
struct NfLivePre {
    NfStream<NF_MLP_NT>& st;
    f32x4 (&wd)[16];
    f32x4 (&pf)[NF_LIVE_PF > 0 ? NF_LIVE_PF : 1];
    char* ring_v;
    int head_v, tail_v;
    // every append of the earlier passes has been acknowledged by L2 before the first load below is issued
    __device__ __forceinline__ void wait() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0x0F70);               // vmcnt(0)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    __device__ __forceinline__ void loads(const NfW& Wi, const NfW& Ci, int lane) {
        using Net = NfPaperNet;
        const __amdgpu_buffer_rsrc_t ring = nf_live_ring(ring_v);
        const int tail = __builtin_amdgcn_readfirstlane(tail_v), cnt = __builtin_amdgcn_readfirstlane(head_v) - tail;
#pragma unroll
        for (int i = 0; i < NF_LIVE_PF; ++i)
            pf[i] = nf_live_load(ring, i < cnt ? ((tail + i) & (NF_LIVE_ROWS - 1)) * 1024 + lane * 16 : NF_LIVE_OOB);
        nf_load_bias<8>(st.bias, Ci, Net::B_D0, lane);
        nf_load_w16<8>(st.wa, Wi, Net::OFF_D0 / 4, lane);
        nf_load_w16<8>(wd, Wi, Net::OFF_D0 / 4 + 16 * 9 * 64, lane);
        __builtin_amdgcn_sched_barrier(0);
    }
};

// GATE: what a pass requests while the bound tile runs alone -- fc_feat's bias and first weight chunk as the gathered run finds them,
// and the oldest ring rows.  The bound image's descriptor is made where it is used, from the pointer's VGPR home.
struct NfGatePre {
    NfStream<NF_MLP_NT>& st;
    f32x4 (&pf)[NF_LIVE_PF > 0 ? NF_LIVE_PF : 1];
    char* ring_v;
    int head_v, tail_v;
    const float* bound_v;
    __device__ __forceinline__ NfW image() const {
        const uint64_t a = (uint64_t)bound_v;
        const uint64_t s = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a) |
                           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32);
        return nf_w_image(reinterpret_cast<const float*>(s), NF_BOUND_FLOATS);
    }
    __device__ __forceinline__ void wait() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0x0F70);               // vmcnt(0)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    __device__ __forceinline__ void loads(const NfW& Wi, const NfW& Ci, int lane) {
        using Net = NfPaperNet;
        const __amdgpu_buffer_rsrc_t ring = nf_live_ring(ring_v);
        const int tail = __builtin_amdgcn_readfirstlane(tail_v), cnt = __builtin_amdgcn_readfirstlane(head_v) - tail;
#pragma unroll
        for (int i = 0; i < NF_LIVE_PF; ++i)
            pf[i] = nf_live_load(ring, i < cnt ? ((tail + i) & (NF_LIVE_ROWS - 1)) * 1024 + lane * 16 : NF_LIVE_OOB);
        nf_load_bias<16>(st.bias, Ci, Net::B_FEAT, lane);
        nf_load_w16<16>(st.wa, Wi, Net::OFF_FEAT / 4, lane);
        __builtin_amdgcn_sched_barrier(0);
    }
};

// What the STATS instantiation writes per wave, row (blockIdx.x * NF_MLP_WAVES + wave) of `stats` (zero when the launch starts):
#define NF_LIVE_STAT_UNITS 0                              // units taken (the one past the end that ends the wave is not counted)
#define NF_LIVE_STAT_RUNS 1                               // colour runs, the final flush included
#define NF_LIVE_STAT_FLUSH 2                              // rows of the final flush
#define NF_LIVE_STAT_CLOCK 3                              // wall_clock64() at exit
#define NF_GATE_STAT_PROVEN 4                             // GATE: rows proven dead (a fifth column; the first four as above, "colour run" =
                                                          // gathered run)
// On request (nf_live_launch's `clocks`: the row is then NF_LIVE_PHASES columns longer) six columns of shader clocks (s_memtime) follow,
// summed over the wave's passes: where a pass spends its time.  The request rides in bit 0 of the kernel's `stats` pointer, which is
// 8-byte aligned: the STATS instantiations alone look at it, and the entry points with the short rows keep their layout.
#define NF_LIVE_PH_TRUNK 0                                // a unit's inputs and the trunk up to the hook (NfLivePre / NfGatePre::wait())
#define NF_LIVE_PH_TILE 1                                 // the hook and the lone tile
#define NF_LIVE_PH_APPEND 2                               // ballot and append
#define NF_LIVE_PH_ENTRY 3                                // a run's gathers and slab fills, up to its first MFMA
#define NF_LIVE_PH_RUN 4                                  // the run and its stores
#define NF_LIVE_PH_DEAD 5                                 // the stores of the rows finished without a colour
#define NF_LIVE_PHASES 6
#define NF_LIVE_STAT_COLS 4
#define NF_GATE_STAT_COLS 5

// one lane of the wave adds to its row; the row belongs to the wave, and nothing is held in a register across the trunk
template <bool STATS, int COLS = NF_LIVE_STAT_COLS>
__device__ __forceinline__ void nf_live_stat(long long* stats, int col, long long add, bool set = false) {
    if constexpr (STATS) {
        const int cols = COLS + (((uintptr_t)stats & 1) ? NF_LIVE_PHASES : 0);
        stats = reinterpret_cast<long long*>((uintptr_t)stats & ~(uintptr_t)7);
        if ((threadIdx.x & 63) == 0) {
            long long* at = stats + ((size_t)blockIdx.x * NF_MLP_WAVES + (threadIdx.x >> 6)) * cols + col;
            if (set) *at = add;                           // (an add that returns nothing: no load, no wait for it in the middle of a pass)
            else (void)__hip_atomic_fetch_add(at, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// STATS: one reading of the shader clock ends phase `end` and starts phase `start` (NF_LIVE_PH_*, -1: none).  A phase's column is the
// sum of its ends minus the sum of its starts, so a mark is two adds that return nothing: no load, no wait, no register kept.
template <bool STATS, int COLS>
__device__ __forceinline__ void nf_live_mark(long long* stats, int end, int start) {
    if constexpr (STATS) {
        if ((uintptr_t)stats & 1) {
            __builtin_amdgcn_sched_barrier(0);
            const long long t = (long long)__builtin_amdgcn_s_memtime();
            if ((threadIdx.x & 63) == 0) {
                long long* row = reinterpret_cast<long long*>((uintptr_t)stats & ~(uintptr_t)7) +
                                 ((size_t)blockIdx.x * NF_MLP_WAVES + (threadIdx.x >> 6)) * (COLS + NF_LIVE_PHASES) + COLS;
                if (end >= 0) (void)__hip_atomic_fetch_add(row + end, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (start >= 0) (void)__hip_atomic_fetch_add(row + start, -t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}
// the hooks of the STATS instantiations: the same requests, behind a mark where the trunk ends
template <class Pre, int COLS>
struct NfMarkedPre : Pre {
    long long* stats;
    __device__ __forceinline__ void wait() const {
        nf_live_mark<true, COLS>(stats, NF_LIVE_PH_TRUNK, NF_LIVE_PH_TILE);
        Pre::wait();
    }
};

// GATE: the kernel of nf_mlp_gated.hip; `bound` is the sigma-bound image of `packed` (not read otherwise).
template <int NT, bool STATS, bool GATE = false>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_paper_mlp_fwd_live(const float* __restrict__ packed, const float* __restrict__ cond_, const float* __restrict__ ro,
                     const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z,
                     int64_t n_points, int S, float* __restrict__ raw, float* __restrict__ scratch, unsigned* __restrict__ counter,
                     long long* __restrict__ stats, const float* __restrict__ bound) {
    using Net = NfPaperNet;
    constexpr int COLS = GATE ? NF_GATE_STAT_COLS : NF_LIVE_STAT_COLS;
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4* act4 = lds + wave * (16 * NT * 64);
    typedef __attribute__((address_space(1))) f32x4 nf_gf32x4;
    // loop invariants and the ring's fill state live in VGPRs, as in k_paper_mlp_fwd: the layer stream leaves no scalar registers
    nf_gf32x4* raw_v = (nf_gf32x4*)raw;
    asm volatile("" : "+v"(raw_v));
    char* ring_v = reinterpret_cast<char*>(scratch) + ((size_t)blockIdx.x * NF_MLP_WAVES + wave) * NF_LIVE_WAVE_B;
    asm volatile("" : "+v"(ring_v));
    const float* z_v = z;
    const float* rdv_v = rd_view;
    asm volatile("" : "+v"(z_v), "+v"(rdv_v));
    const float* bound_v = bound;
    if constexpr (GATE) asm volatile("" : "+v"(bound_v));
    int head_v = 0, tail_v = 0;                           // rows appended / consumed so far (row = count & 63); head - tail <= 31
    asm volatile("" : "+v"(head_v), "+v"(tail_v));
    // Unit u is points 32 u .. 32 u + 31, and a wave takes its units from the launch's counter (zero when the launch starts), one at
    // a time, in whatever order the waves come for them: how long a unit takes depends on whether its pass ends in a colour run,
    // which depends on where the object is, and with a fixed share of the units per wave the launch ended with the wave whose
    // share held the most runs.  Lane 0 adds; the value waits in its VGPR until the wave needs it as a scalar.
    typedef __attribute__((address_space(1))) unsigned nf_gu32;       // (a global_, not a flat_ atomic: it must not count as an LDS access)
    nf_gu32* ctr_v = (nf_gu32*)counter;
    asm volatile("" : "+v"(ctr_v));
    unsigned unit_v = 0;
    if (lane == 0) unit_v = __hip_atomic_fetch_add(ctr_v, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // atomicAdd
    asm volatile("" : "+v"(unit_v));
#pragma unroll 1
    for (;;) {
        const int64_t p0 = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)unit_v) * (16 * NT);
        int64_t p0_v = p0;                                // (its home across the trunk and the colour run)
        asm volatile("" : "+v"(p0_v));
        int more_v = p0 < n_points;                       // wave-uniform; no barriers anywhere below
        asm volatile("" : "+v"(more_v));
        const bool more = __builtin_amdgcn_readfirstlane(more_v) != 0;
        // the unit after this one is requested here and read at the bottom of the pass: the round trip to the counter runs beside
        // the loads of the pass's inputs and the trunk.  (A wave whose unit is past the end requests nothing more: a launch adds
        // units + waves to the counter.)
        unsigned next_v = 0;
        if (more && lane == 0) next_v = __hip_atomic_fetch_add(ctr_v, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (more) nf_live_stat<STATS, COLS>(stats, NF_LIVE_STAT_UNITS, 1);
        int opaque0 = 0;                                  // per-block opaque zero: the weight / bias loads must stay where the layers issue them
        asm volatile("" : "+s"(opaque0));
        const NfW Wi = nf_w_image(packed + opaque0, Net::PACKED), Ci = nf_w_image(cond_ + opaque0, Net::COND_FLOATS);
        NfStream<NT> st;
        f32x4 wd[16], pf[NF_LIVE_PF > 0 ? NF_LIVE_PF : 1];
        f32x4 dirf[NT][1];
        float sigma_own[NT];
        // GATE: sigma_own is the bound s + 2^-13 u of the pass's own rows -- what a proven row gets for its density -- and "live" reads
        // "not proven dead"; tag_own is nonzero bits on a ray's last sample (the third word of a meta row, in sigma_raw's place: the
        // gathered run computes the density itself and needs to know whether a row that turns out dead keeps its colour)
        float tag_own[NT] = {};
        bool proven[NT] = {};
        int live_v = 0, run_v = 0;                        // the pass's 32-bit liveness mask; nonzero: the colour layers run
        if (more) {
            nf_live_mark<STATS, COLS>(stats, -1, NF_LIVE_PH_TRUNK);
            f32x4 pe[NT][4];
            nf_net_inputs<NT>(pe, dirf, p0, n_points, S, lane, ro, rd, rdv_v, z_v);
            f32x4 acc[NT][16];
            if constexpr (GATE) {
                if constexpr (STATS)
                    nf_paper_net_body<Net, NT, 1, true, NfMarkedPre<NfGatePre, COLS>, true>(
                        acc, sigma_own, pe, dirf, Wi, Ci, act4, lane, NfMarkedPre<NfGatePre, COLS>{{st, pf, ring_v, head_v, tail_v, bound_v}, stats});
                else
                    nf_paper_net_body<Net, NT, 1, true, NfGatePre, true>(acc, sigma_own, pe, dirf, Wi, Ci, act4, lane,
                                                                         NfGatePre{st, pf, ring_v, head_v, tail_v, bound_v});
#pragma unroll
                for (int t = 0; t < NT; ++t) {             // proven dead iff s + 2^-13 u < -2^-100, false for NaN or infinite operands
                    const float s = acc[t][8].x, u = acc[t][8].y;
                    sigma_own[t] = nf_add(s, nf_mul(u, 0x1p-13f));
                    proven[t] = sigma_own[t] < -0x1p-100f && s > -INFINITY && u < INFINITY;
                }
            } else if constexpr (STATS) {
                nf_paper_net_body<Net, NT, 1, true>(acc, sigma_own, pe, dirf, Wi, Ci, act4, lane,
                                                    NfMarkedPre<NfLivePre, COLS>{{st, wd, pf, ring_v, head_v, tail_v}, stats});
            } else {
                nf_paper_net_body<Net, NT, 1, true>(acc, sigma_own, pe, dirf, Wi, Ci, act4, lane, NfLivePre{st, wd, pf, ring_v, head_v, tail_v});
            }
            nf_live_mark<STATS, COLS>(stats, NF_LIVE_PH_TILE, NF_LIVE_PH_APPEND);
            int lane_o = lane;
            asm volatile("" : "+v"(lane_o));
            const int g = lane_o >> 4, c = lane_o & 15;
            // lane group 0 holds sigma_raw of point 16 t + c: liveness as one 16-bit mask per tile
            unsigned live = 0;
            int S_o = S;                                  // (opaque: nothing derived from S is hoisted out of the block loop)
            asm volatile("" : "+v"(S_o));
            const int64_t p0_o = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)p0_v) |
                                 ((int64_t)__builtin_amdgcn_readfirstlane((int)(p0_v >> 32)) << 32);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int64_t p = p0_o + 16 * t + c;
                bool is_live;
                if constexpr (GATE) {                     // (the 64-bit remainder once: it is some 300 clocks of vector work per tile)
                    const bool last = (p + 1) % S_o == 0;
                    is_live = g == 0 && p < n_points && (!proven[t] || last);
                    tag_own[t] = __int_as_float(last ? 1 : 0);
                } else {
                    is_live = g == 0 && p < n_points && (!(sigma_own[t] <= 0.0f) || (p + 1) % S_o == 0);
                }
                live |= ((unsigned)__builtin_amdgcn_ballot_w64(is_live) & 0xffffu) << (16 * t);
            }
            const int head = __builtin_amdgcn_readfirstlane(head_v), cnt = head - __builtin_amdgcn_readfirstlane(tail_v);
            const int n_live = __builtin_popcount(live);
            live_v = (int)live;
            if constexpr (GATE) {                         // (in-range rows that are not kept are the proven ones)
                const int64_t left = n_points - p0_o;
                nf_live_stat<STATS, COLS>(stats, NF_GATE_STAT_PROVEN, (left < 16 * NT ? (int)left : 16 * NT) - n_live);
            }
            if (cnt + n_live >= 16 * NT) {                // the ring fills every hole
                run_v = 1;
            } else {                                      // append the live rows; nothing runs
                const __amdgpu_buffer_rsrc_t ring = nf_live_ring(ring_v);
                unsigned mm = live;
#pragma unroll 1
                for (int i = 0; i < n_live; i += 4) {
                    f32x4 v[4];
                    int off[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool ok = i + u < n_live;
                        const int r = ok ? nf_live_pop(mm) : 0;
                        off[u] = ok ? ((head + i + u) & (NF_LIVE_ROWS - 1)) * 1024 + lane_o * 16 : NF_LIVE_OOB;
                        v[u] = act4[nf_live_slab(r, lane_o)];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) nf_live_store(ring, off[u], v[u]);
                }
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int bit = 16 * t + c;
                    if ((live >> bit) & 1u) {
                        const int row = (head + __builtin_popcount(live & ((1u << bit) - 1u))) & (NF_LIVE_ROWS - 1);
                        nf_live_store(ring, NF_LIVE_DIR_B + row * 64 + g * 16, dirf[t][0]);
                        if (g == 0) {
                            const int64_t p = p0_o + bit;
                            nf_live_store(ring, NF_LIVE_META_B + row * 16,
                                          (f32x4){__int_as_float((int)(uint32_t)p), __int_as_float((int)(p >> 32)), GATE ? tag_own[t] : sigma_own[t], 0.0f});
                        }
                    }
                }
                head_v = head + n_live;
                asm volatile("" : "+v"(head_v));
            }
            nf_live_mark<STATS, COLS>(stats, NF_LIVE_PH_APPEND, -1);
        } else {
            // behind the wave's last block: what the ring holds goes to rows 0 .. R - 1 of the slab.  (The requests are made with an
            // empty ring too, once per wave: every path into the colour run below defines what it reads.)
            if constexpr (GATE) {
                NfGatePre pre{st, pf, ring_v, head_v, tail_v, bound_v};
                pre.wait();
                pre.loads(Wi, Ci, lane);
            } else {
                NfLivePre pre{st, wd, pf, ring_v, head_v, tail_v};
                pre.wait();
                pre.loads(Wi, Ci, lane);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                dirf[t][0] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                sigma_own[t] = 0.0f;
            }
            run_v = __builtin_amdgcn_readfirstlane(head_v) != __builtin_amdgcn_readfirstlane(tail_v) ? 2 : 0;
        }
        asm volatile("" : "+v"(live_v), "+v"(run_v));
        const int run = __builtin_amdgcn_readfirstlane(run_v);
        if (run != 0) {
            nf_live_stat<STATS, COLS>(stats, NF_LIVE_STAT_RUNS, 1);
            if (run == 2) nf_live_stat<STATS, COLS>(stats, NF_LIVE_STAT_FLUSH, __builtin_amdgcn_readfirstlane(head_v) - __builtin_amdgcn_readfirstlane(tail_v));
            nf_live_mark<STATS, COLS>(stats, -1, NF_LIVE_PH_ENTRY);
            int lane_o = lane;
            asm volatile("" : "+v"(lane_o));
            const int g = lane_o >> 4, c = lane_o & 15;
            const __amdgpu_buffer_rsrc_t ring = nf_live_ring(ring_v);
            const int tail = __builtin_amdgcn_readfirstlane(tail_v), cnt = __builtin_amdgcn_readfirstlane(head_v) - tail;
            const unsigned own = run == 1 ? (unsigned)__builtin_amdgcn_readfirstlane(live_v) : 0u;      // rows that stay as they are
            const unsigned fill = run == 1 ? ~own : (1u << cnt) - 1u;                                    // rows the ring fills, oldest first
            const int n_fill = __builtin_popcount(fill);
            // index, direction fragment and sigma_raw of a filled row, gathered per lane
            f32x4 meta[NT];
            bool valid[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int bit = 16 * t + c;
                const bool f = (fill >> bit) & 1u;
                const int row = (tail + __builtin_popcount(fill & ((1u << bit) - 1u))) & (NF_LIVE_ROWS - 1);
                const f32x4 fd = nf_live_load(ring, f ? NF_LIVE_DIR_B + row * 64 + g * 16 : NF_LIVE_OOB);
                const f32x4 fm = nf_live_load(ring, f ? NF_LIVE_META_B + row * 16 : NF_LIVE_OOB);
                const int64_t p = (p0_v) + bit;
                dirf[t][0] = f ? fd : dirf[t][0];
                meta[t] = f ? fm : (f32x4){__int_as_float((int)(uint32_t)p), __int_as_float((int)(p >> 32)), GATE ? tag_own[t] : sigma_own[t], 0.0f};
                valid[t] = f || ((own >> bit) & 1u);
            }
            // the rows themselves: the prefetched ones from their registers, the others loaded here
            unsigned hh = fill;
#pragma unroll
            for (int i = 0; i < NF_LIVE_PF; ++i) {
                if (i < n_fill) {
                    const int h = nf_live_pop(hh);
                    act4[nf_live_slab(h, lane_o)] = pf[i];
                }
            }
#pragma unroll 1
            for (int i = NF_LIVE_PF; i < n_fill; i += 4) {
                f32x4 v[4];
                int h[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool ok = i + u < n_fill;
                    h[u] = ok ? nf_live_pop(hh) : -1;
                    v[u] = nf_live_load(ring, ok ? ((tail + i + u) & (NF_LIVE_ROWS - 1)) * 1024 + lane_o * 16 : NF_LIVE_OOB);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (h[u] >= 0) act4[nf_live_slab(h[u], lane_o)] = v[u];
            }
            // layers_dir.0 starts as a layer's tail would leave it: bias and first weight chunk requested (NfLivePre), first B fragment
            // as stored.  Output tiles 0 .. 7 only; the weight image keeps its 9-tile chunk stride.
            // GATE: the slab holds layers_xyz.5's accumulators, and fc_feat starts the same way (NfGatePre); behind it layers_dir.0 in its
            // full nine-tile form, fc_alpha as tile 8: the MFMAs of k_paper_mlp_fwd from fc_feat on, in its order.
            constexpr int NDIR = 1;
            constexpr unsigned D0 = Net::OFF_D0 / 4;
            nf_read_b<NT>(st.b0, act4, lane, 0);
            nf_live_mark<STATS, COLS>(stats, NF_LIVE_PH_ENTRY, NF_LIVE_PH_RUN);
            f32x4 acc[NT][16], bj[NT];
            float sigma_raw[NT];
            if constexpr (GATE) {
                nf_seg_lds<NT, 16, true, true>(acc, st, Wi, Net::OFF_FEAT / 4, 16, act4, lane);
                nf_pending_b<NT, true>(bj, st);
                nf_tail<NT, 16, 16, 9, 1>(acc, st.wb, bj, st, Wi, D0, Ci, Net::B_D0, act4, lane);
                NF_NET_COLOUR();
            } else {
                NF_NET_COLOUR_D0(8, 9, wd);
                NF_NET_COLOUR_REST();
            }
            int lane_s = lane;
            asm volatile("" : "+v"(lane_s));
            if ((lane_s >> 4) == 0) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (valid[t]) {
                        const int64_t p = (int64_t)(uint32_t)__float_as_int(meta[t].x) | ((int64_t)__float_as_int(meta[t].y) << 32);
                        if constexpr (GATE) {             // a gathered row that turns out dead: rgb 0 and its exact density
                            const bool keep = !(sigma_raw[t] <= 0.0f) || __float_as_int(meta[t].z) != 0;
                            if (p >= 0 && p < n_points)
                                raw_v[p] = (f32x4){keep ? acc[t][0].x : 0.0f, keep ? acc[t][0].y : 0.0f, keep ? acc[t][0].z : 0.0f, sigma_raw[t]};
                        } else {
                            if (p >= 0 && p < n_points) raw_v[p] = (f32x4){acc[t][0].x, acc[t][0].y, acc[t][0].z, meta[t].z};
                        }
                    }
                }
            }
            tail_v = tail + n_fill;
            asm volatile("" : "+v"(tail_v));
            nf_live_mark<STATS, COLS>(stats, NF_LIVE_PH_RUN, -1);
        }
        asm volatile("" : "+v"(more_v));
        if (__builtin_amdgcn_readfirstlane(more_v) == 0) break;
        {   // the dead points of the block: finished without a colour
            nf_live_mark<STATS, COLS>(stats, -1, NF_LIVE_PH_DEAD);
            int lane_s = lane;
            asm volatile("" : "+v"(lane_s));
            const int g = lane_s >> 4, c = lane_s & 15;
            asm volatile("" : "+v"(live_v));
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int64_t p = p0_v + 16 * t + c;
                if (g == 0 && p < n_points && !(((unsigned)live_v >> (16 * t + c)) & 1u)) raw_v[p] = (f32x4){0.0f, 0.0f, 0.0f, sigma_own[t]};
            }
            nf_live_mark<STATS, COLS>(stats, NF_LIVE_PH_DEAD, -1);
        }
        asm volatile("" : "+v"(next_v));
        unit_v = next_v;
    }
    nf_live_stat<STATS, COLS>(stats, NF_LIVE_STAT_CLOCK, (long long)wall_clock64(), true);
}

// a grid capped at max_workgroups (0: one workgroup per CU of the current device)
static inline int64_t nf_live_grid_cap(int max_workgroups) {
    const int64_t cu = nf_cu_count();
    return max_workgroups > 0 && max_workgroups < cu ? max_workgroups : cu;
}

// The unit counters of the launches, in device memory the library owns: one block of NF_LIVE_SLOTS counters per device (a
// 128-byte line each), allocated at the first launch on that device and kept for the life of the process; no later launch allocates.
// A STREAM owns a slot, from its first launch on: a launch zeroes the stream's slot with a 4-byte memset on that stream and starts
// the kernel behind it.  Reuse of a slot is therefore ordered by the stream itself: the memset of launch n + 1 runs behind the kernel
// of launch n, however closely the host issues them, and a captured graph replays memset and kernel in that order.  Two launches can
// only be in flight together on two streams, which hold two slots.  hipStreamPerThread is a different stream in every host thread
// and is keyed by the thread.  A table that is full (NF_LIVE_SLOTS distinct streams on one device) is emptied behind a
// hipDeviceSynchronize(): with nothing in flight every slot is free.  nullptr: the allocation or that synchronise failed.
#define NF_LIVE_SLOTS 256
#define NF_LIVE_SLOT_B 128

inline unsigned* nf_live_counter(hipStream_t stream) {
    struct Pool {
        char* base;
        const void* owner[NF_LIVE_SLOTS];
        int used;
    };
    static std::mutex mu;
    static Pool pools[64];
    static thread_local char this_thread;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    const void* key = stream == hipStreamPerThread ? (const void*)&this_thread : (const void*)stream;
    std::lock_guard<std::mutex> lock(mu);
    Pool& p = pools[dev];
    if (!p.base) {
        void* mem = nullptr;
        if (hipMalloc(&mem, (size_t)NF_LIVE_SLOTS * NF_LIVE_SLOT_B) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        p.base = (char*)mem;
        p.used = 0;
    }
    int i = 0;
    while (i < p.used && p.owner[i] != key) ++i;
    if (i == p.used) {
        if (p.used == NF_LIVE_SLOTS) {
            if (hipDeviceSynchronize() != hipSuccess) return nullptr;
            p.used = i = 0;
        }
        p.owner[p.used++] = key;
    }
    return reinterpret_cast<unsigned*>(p.base + (size_t)i * NF_LIVE_SLOT_B);
}

// Argument checks and launch of either instantiation (stats: null for the production kernel).  A unit number is 32 bits wide and the
// counter ends at units + waves: more than 2^31 units (2^36 points) are refused.
template <bool STATS, bool GATE = false>
static inline int nf_live_launch(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view, const float* z,
                                 int64_t n_rays, int n_samples, float* raw, float* scratch, size_t scratch_floats, int max_workgroups,
                                 long long* stats, nf_stream_t stream, const float* bound = nullptr, bool clocks = false) {
    static_assert(NF_MLP_WAVES * 16 * NF_MLP_NT == 128, "nf_mlp_fwd_launch sizes the grid for 128 points per workgroup");
    if (max_workgroups < 0 || !scratch || ((uintptr_t)scratch & 15) ||
        scratch_floats < (size_t)nf_live_grid_cap(max_workgroups) * NF_MLP_WAVES * (NF_LIVE_WAVE_B / 4) ||
        (GATE && (!bound || ((uintptr_t)bound & 15))))
        return NF_EINVAL;
    const float* rdv = rd_view ? rd_view : rd;
    if (STATS && clocks) stats = reinterpret_cast<long long*>((uintptr_t)stats | 1);      // (a request for the clock columns: see NF_LIVE_PH_*)
    int rc = 0;
    const int launched = nf_mlp_fwd_launch(NF_FWD_INFER, packed, cond, ro, rd, z, raw, nullptr, n_rays, n_samples, [&](int64_t n_points, unsigned grid) {
        if ((n_points + 31) / 32 > ((int64_t)1 << 31)) {
            rc = NF_EINVAL;
            return;
        }
        unsigned* counter = nf_live_counter(nf_s(stream));
        if (!counter) {
            rc = (int)hipErrorOutOfMemory;
            return;
        }
        const hipError_t e = hipMemsetAsync(counter, 0, sizeof(unsigned), nf_s(stream));
        if (e != hipSuccess) {
            rc = (int)e;
            return;
        }
        const int64_t cap = nf_live_grid_cap(max_workgroups);
        hipLaunchKernelGGL((k_paper_mlp_fwd_live<NF_MLP_NT, STATS, GATE>), dim3((unsigned)(grid < cap ? grid : cap)), dim3(64 * NF_MLP_WAVES), 0,
                           nf_s(stream), packed, cond, ro, rd, rdv, z, n_points, n_samples, raw, scratch, counter, stats, bound);
    });
    return rc ? rc : launched;
}
