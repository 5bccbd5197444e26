// Exact-f32 inference forward of ConditionalBlendshapePaperNeRFModel that runs the colour layers only on samples the integrator can
// see: k_paper_mlp_fwd (nf_mlp.hip) with layers_dir.0 .. fc_rgb taken off the dead points.  A translation unit of its own: the
// objects of the other kernels do not change.
//
// A sample whose raw density is <= 0 has alpha = 1 - exp(-0 * dist) = 0 exactly, so the integrator multiplies its colour by an exact
// zero in every output; only the last sample of a ray (1e-6 is added to its density) and a NaN density keep their colour visible.
// Such a point is LIVE: !(sigma_raw <= 0) or p % S == S - 1.  Every other point is dead and gets rgb_raw = 0.
//
// Same persistent grid as k_paper_mlp_fwd (one workgroup per CU, four independent waves, 32 points per wave pass, no barrier).  A pass:
//   1. the trunk through fc_feat and fc_alpha alone (nf_paper_net_body<..., SIGMA>): feat of the 32 points in the wave's LDS slab,
//      sigma_raw in registers; dead points are finished here -- (0, 0, 0, sigma_raw) goes to `raw`;
//   2. live points are appended to the wave's ring of 64 rows in `scratch` (global memory) at ranks taken from a ballot and a prefix
//      count: feat as the lane's own B fragments (1 KiB), the direction fragments (64 B), the point index;
//   3. once the ring holds 32 rows they are read back into the slab and layers_dir.0 .. fc_rgb run on them with the ordinary stream
//      (NF_NET_COLOUR; tile 8 of layers_dir.0 is computed again, so sigma_raw comes out exactly as the full kernel has it) and
//      (r, g, b, sigma_raw) are scattered to `raw` by point index.  31 + 32 < 64: at most one colour run is due per pass.
// After its last block a wave runs the colour layers on what is left, padded to 32 with whatever the ring holds: MFMA columns are
// independent per point, and only the valid ones are stored.  Every point of `raw` is written exactly once.
//
// Ring coherence.  Rows are written and read by the same wave, but by different lanes.  Between the appends and the read-back stands a
// workgroup-scope release / acquire fence pair around an explicit s_waitcnt vmcnt(0) (at workgroup scope the fences alone rely on the
// vector cache keeping one CU's accesses in order and emit no wait): every store has been acknowledged by L2 before a load is issued.
// The read-back loads carry sc1 (agent scope): they are served by that L2, where the write-through stores of this CU have landed,
// never by a line the per-CU vector cache kept from an earlier lap of the ring.  All ring traffic goes through a buffer descriptor
// that covers exactly the wave's ring: an index outside it would be dropped by the range check, not written.
#include "nf_mlp_paper_net.h"

#define NF_LIVE_ROWS 64                                   // ring rows per wave
#define NF_LIVE_DIR_B (NF_LIVE_ROWS * 1024)               // byte offsets inside a wave's ring: [rows][64] feat fragments, then
#define NF_LIVE_META_B (NF_LIVE_DIR_B + NF_LIVE_ROWS * 64)     // [rows][4] direction fragments, then [rows] (index lo, hi, -, -)
#define NF_LIVE_WAVE_B (NF_LIVE_META_B + NF_LIVE_ROWS * 16)
#define NF_LIVE_SC1 16                                    // cache policy bit of the buffer loads: sc1

static_assert(NF_LIVE_ROWS == 64 && NF_MLP_NT == 2, "ranks wrap with & 63; 31 left over + 32 appended must fit");

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

template <int NT>
__global__ void __launch_bounds__(64 * NF_MLP_WAVES, 1)
k_paper_mlp_fwd_live(const float* __restrict__ packed, const float* __restrict__ cond_, const float* __restrict__ ro,
                     const float* __restrict__ rd, const float* __restrict__ rd_view, const float* __restrict__ z,
                     int64_t n_points, int S, float* __restrict__ raw, float* __restrict__ scratch) {
    using Net = NfPaperNet;
    __shared__ __attribute__((aligned(16))) f32x4 lds[NF_MLP_WAVES * 16 * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4* act4 = lds + wave * (16 * NT * 64);
    typedef __attribute__((address_space(1))) f32x4 nf_gf32x4;
    // loop invariants and the ring's fill state live in VGPRs, as in k_paper_mlp_fwd: the layer stream leaves no scalar registers
    nf_gf32x4* raw_v = (nf_gf32x4*)raw;
    asm volatile("" : "+v"(raw_v));
    int stride_v = (int)gridDim.x;
    asm volatile("" : "+v"(stride_v));
    char* ring_v = reinterpret_cast<char*>(scratch) + ((size_t)blockIdx.x * NF_MLP_WAVES + wave) * NF_LIVE_WAVE_B;
    asm volatile("" : "+v"(ring_v));
    const float* z_v = z;
    const float* rdv_v = rd_view;
    asm volatile("" : "+v"(z_v), "+v"(rdv_v));
    int head_v = 0, tail_v = 0;                           // rows appended / consumed so far (row = count & 63)
    asm volatile("" : "+v"(head_v), "+v"(tail_v));
    // Pass k of workgroup b takes block k G + (b + k R) mod G of the G = gridDim.x blocks of that pass, not block k G + b: with a fixed
    // b a workgroup would see the same few image columns in every pass (a 65536 x 64 launch: G blocks = one image row), and the
    // colour work, which depends on where the object is, would pile up on the workgroups of the columns that cross it.
    int rot_v = (int)blockIdx.x, step_v = ((int)gridDim.x * 5 / 13) | 1;
    if (step_v >= (int)gridDim.x) step_v = 0;             // (one workgroup)
    asm volatile("" : "+v"(rot_v), "+v"(step_v));
#pragma unroll 1
    for (int64_t base = 0;; base += __builtin_amdgcn_readfirstlane(stride_v)) {
        const int64_t blk = base + __builtin_amdgcn_readfirstlane(rot_v);
        {
            const int g_n = __builtin_amdgcn_readfirstlane(stride_v);
            int r = __builtin_amdgcn_readfirstlane(rot_v) + __builtin_amdgcn_readfirstlane(step_v);
            rot_v = r >= g_n ? r - g_n : r;
            asm volatile("" : "+v"(rot_v));
        }
        const int64_t p0 = (blk * NF_MLP_WAVES + wave) * (16 * NT);
        int more_v = p0 < n_points;                       // wave-uniform; no barriers anywhere below
        asm volatile("" : "+v"(more_v));
        const bool more = __builtin_amdgcn_readfirstlane(more_v) != 0;
        int opaque0 = 0;                                  // per-block opaque zero: the weight / bias loads must stay where the layers issue them
        asm volatile("" : "+s"(opaque0));
        const NfW Wi = nf_w_image(packed + opaque0, Net::PACKED), Ci = nf_w_image(cond_ + opaque0, Net::COND_FLOATS);
        if (more) {
            f32x4 pe[NT][4];
            f32x4 dirf[NT][1];
            nf_net_inputs<NT>(pe, dirf, p0, n_points, S, lane, ro, rd, rdv_v, z_v);
            f32x4 acc[NT][16];
            float sigma_raw[NT];
            nf_paper_net_body<Net, NT, 1, true>(acc, sigma_raw, pe, dirf, Wi, Ci, act4, lane);
            int lane_o = lane;
            asm volatile("" : "+v"(lane_o));
            const int g = lane_o >> 4, c = lane_o & 15;
            const __amdgpu_buffer_rsrc_t ring = nf_live_ring(ring_v);
            // lane group 0 holds sigma_raw of point 16 t + c: liveness as one 16-bit mask per tile
            unsigned m[NT];
            int S_o = S;                                  // (opaque: nothing derived from S is hoisted out of the block loop)
            asm volatile("" : "+v"(S_o));
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int64_t p = p0 + 16 * t + c;
                const bool mine = g == 0 && p < n_points;
                const bool live = mine && (!(sigma_raw[t] <= 0.0f) || (p + 1) % S_o == 0);
                m[t] = (unsigned)__builtin_amdgcn_ballot_w64(live) & 0xffffu;
                if (mine && !live) raw_v[p] = (f32x4){0.0f, 0.0f, 0.0f, sigma_raw[t]};
            }
            int rows = __builtin_amdgcn_readfirstlane(head_v);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if ((m[t] >> c) & 1u) {                   // every lane group copies its own fragments of the point
                    const int row = (rows + __builtin_popcount(m[t] & ((1u << c) - 1u))) & (NF_LIVE_ROWS - 1);
                    f32x4 v[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) v[j] = act4[nf_act_idx4(16 * t + c, 4 * j + g)];
#pragma unroll
                    for (int j = 0; j < 16; ++j) nf_live_store(ring, row * 1024 + (4 * j + g) * 16, v[j]);
                    nf_live_store(ring, NF_LIVE_DIR_B + row * 64 + g * 16, dirf[t][0]);
                    if (g == 0) {
                        const int64_t p = p0 + 16 * t + c;
                        nf_live_store(ring, NF_LIVE_META_B + row * 16,
                                      (f32x4){__int_as_float((int)(uint32_t)p), __int_as_float((int)(p >> 32)), 0.0f, 0.0f});
                    }
                }
                rows += __builtin_popcount(m[t]);
            }
            head_v = rows;
            asm volatile("" : "+v"(head_v));
        }
        asm volatile("" : "+v"(more_v));                  // (read again: not kept in a scalar register across the trunk)
        const bool last = __builtin_amdgcn_readfirstlane(more_v) == 0;
        const int head = __builtin_amdgcn_readfirstlane(head_v), tail = __builtin_amdgcn_readfirstlane(tail_v);
        const int cnt = head - tail;
        if (cnt >= 16 * NT || (last && cnt > 0)) {
            const int n_valid = cnt < 16 * NT ? cnt : 16 * NT;
            int lane_o = lane;
            asm volatile("" : "+v"(lane_o));
            const int g = lane_o >> 4, c = lane_o & 15;
            const __amdgpu_buffer_rsrc_t ring = nf_live_ring(ring_v);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_s_waitcnt(0x0F70);           // vmcnt(0): every append has been acknowledged by L2
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            f32x4 dirf[NT][1], meta[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int row = (tail + 16 * t + c) & (NF_LIVE_ROWS - 1);
                f32x4 v[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = nf_live_load(ring, row * 1024 + (4 * j + g) * 16);
#pragma unroll
                for (int j = 0; j < 16; ++j) act4[nf_act_idx4(16 * t + c, 4 * j + g)] = v[j];
                dirf[t][0] = nf_live_load(ring, NF_LIVE_DIR_B + row * 64 + g * 16);
                meta[t] = nf_live_load(ring, NF_LIVE_META_B + row * 16);
            }
            // layers_dir.0 starts as nf_tail leaves it in the full kernel: bias, first weight chunk, first B fragment as stored
            constexpr int NDIR = 1;
            constexpr unsigned D0 = Net::OFF_D0 / 4;
            NfStream<NT> st;
            nf_load_bias<9>(st.bias, Ci, Net::B_D0, lane);
            nf_load_w16<9>(st.wa, Wi, D0, lane);
            nf_read_b<NT>(st.b0, act4, lane, 0);
            f32x4 acc[NT][16], bj[NT];
            float sigma_raw[NT];
            NF_NET_COLOUR();
            int lane_s = lane;
            asm volatile("" : "+v"(lane_s));
            if ((lane_s >> 4) == 0) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (16 * t + (lane_s & 15) < n_valid) {
                        const int64_t p = (int64_t)(uint32_t)__float_as_int(meta[t].x) | ((int64_t)__float_as_int(meta[t].y) << 32);
                        if (p >= 0 && p < n_points) raw_v[p] = (f32x4){acc[t][0].x, acc[t][0].y, acc[t][0].z, sigma_raw[t]};
                    }
                }
            }
            tail_v = tail + n_valid;
            asm volatile("" : "+v"(tail_v));
        }
        asm volatile("" : "+v"(more_v));
        if (__builtin_amdgcn_readfirstlane(more_v) == 0) break;
    }
}

// floats of `scratch` for a grid capped at max_workgroups (0: one workgroup per CU of the current device)
static int64_t nf_live_grid_cap(int max_workgroups) {
    const int64_t cu = nf_cu_count();
    return max_workgroups > 0 && max_workgroups < cu ? max_workgroups : cu;
}

extern "C" size_t nf_paper_mlp_fwd_live_scratch_floats(int max_workgroups) {
    return (size_t)nf_live_grid_cap(max_workgroups) * NF_MLP_WAVES * (NF_LIVE_WAVE_B / 4);
}

extern "C" int nf_paper_mlp_fwd_live(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                     const float* z, int64_t n_rays, int n_samples, float* raw, float* scratch, size_t scratch_floats,
                                     int max_workgroups, nf_stream_t stream) {
    static_assert(NF_MLP_WAVES * 16 * NF_MLP_NT == 128, "nf_mlp_fwd_launch sizes the grid for 128 points per workgroup");
    if (max_workgroups < 0 || !scratch || ((uintptr_t)scratch & 15) || scratch_floats < nf_paper_mlp_fwd_live_scratch_floats(max_workgroups))
        return NF_EINVAL;
    const float* rdv = rd_view ? rd_view : rd;
    return nf_mlp_fwd_launch(NF_FWD_INFER, packed, cond, ro, rd, z, raw, nullptr, n_rays, n_samples, [&](int64_t n_points, unsigned grid) {
        const int64_t cap = nf_live_grid_cap(max_workgroups);
        hipLaunchKernelGGL(k_paper_mlp_fwd_live<NF_MLP_NT>, dim3((unsigned)(grid < cap ? grid : cap)), dim3(64 * NF_MLP_WAVES), 0, nf_s(stream),
                           packed, cond, ro, rd, rdv, z, n_points, n_samples, raw, scratch);
    });
}
