// Shared helpers for the gfx950 kernels of libnerface_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nerface_hip.h"
#include "nf_sincos.h"

#define NF_WAVE 64

// Launch check: kernels are asynchronous, so this only reports launch-time failures.
#define NF_RETURN_LAUNCH()                         \
    do {                                           \
        hipError_t e__ = hipGetLastError();        \
        return e__ == hipSuccess ? 0 : (int)e__;   \
    } while (0)

static inline hipStream_t nf_s(nf_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Compute units of the CURRENT device (cached per device index: a process may drive several GPUs).  Persistent grids and the
// weight-gradient slice plan are sized from it; without a device (host-only size queries in the CPU tests) it is gfx950's 256.
static inline int64_t nf_cu_count() {
    static int n[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!n[dev]) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        n[dev] = v;
    }
    return n[dev];
}


// Argument check and grid of the fused-MLP forward entry points, before anything touches the device: empty work returns 0, NULL
// pointers or impossible sizes NF_EINVAL; otherwise launch(n_points, grid) runs with one workgroup per 128 points.  The training
// modes require `saved`, whose sections are addressed with 32-bit byte offsets (a larger launch would wrap the buffer descriptor to
// an empty range and drop every save without an error): the exact-f32 layout bounds n_points, the split layout n_points padded to 32.
enum NfFwdMode { NF_FWD_INFER, NF_FWD_TRAIN_F32, NF_FWD_TRAIN_SPLIT };

template <class Launch>
static inline int nf_mlp_fwd_launch(NfFwdMode mode, const void* w, const float* cond, const float* ro, const float* rd, const float* z,
                                    const float* raw, const float* saved, int64_t n_rays, int n_samples, Launch launch) {
    if (n_rays == 0 && n_samples > 0) return 0;            // nothing to do (empty tensors have NULL data pointers)
    if (!w || !cond || !ro || !rd || !z || !raw || (mode != NF_FWD_INFER && !saved) || n_rays < 0 || n_samples <= 0) return NF_EINVAL;
    const int64_t n_points = n_rays * n_samples;
    if (n_points == 0) return 0;
    const int64_t grid = (n_points + 127) / 128;
    if (grid > 0x7fffffff) return NF_EINVAL;
    const int64_t section = mode == NF_FWD_TRAIN_SPLIT ? (n_points + 31) & ~(int64_t)31 : n_points;
    if (mode != NF_FWD_INFER && section >= ((int64_t)1 << 22)) return NF_EINVAL;
    launch(n_points, (unsigned)grid);
    NF_RETURN_LAUNCH();
}

// IEEE single ops that must not be contracted into FMAs (bit parity with the reference's
// separate mul / add tensor ops).  The library is also built with -ffp-contract=off.
__device__ __forceinline__ float nf_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float nf_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float nf_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float nf_div(float a, float b) { return __fdiv_rn(a, b); }
