// K1 ray generation, K2 stratified coarse sampler, K3 stand-alone positional encoder.
// All three are HBM-bound streaming kernels: one thread per output vector, coalesced stores.
#include "nf_common.h"

// ---------------------------------------------------------------------------------------------
// K1: get_ray_bundle (reference nerf/nerf_helpers.py:68-123).  One thread per pixel.
//   dir = ((w - cx_w)/fx, -((h - cy_h)/fy), -1);  rd_i = (dx*R[i,0] + dy*R[i,1]) + dz*R[i,2]
// The association order and the true divisions reproduce the reference bit for bit.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ray_bundle(int height, int width, float fx, float fy, float cx_w,
                                                    float cy_h, const float* __restrict__ c2w, int rs,
                                                    float* __restrict__ ro, float* __restrict__ rd) {
    const int64_t n = (int64_t)height * width;
    const float r00 = c2w[0], r01 = c2w[1], r02 = c2w[2], t0 = c2w[3];
    const float r10 = c2w[rs + 0], r11 = c2w[rs + 1], r12 = c2w[rs + 2], t1 = c2w[rs + 3];
    const float r20 = c2w[2 * rs + 0], r21 = c2w[2 * rs + 1], r22 = c2w[2 * rs + 2], t2 = c2w[2 * rs + 3];
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int h = (int)(p / width), w = (int)(p - (int64_t)h * width);
        const float dx = nf_div(nf_sub((float)w, cx_w), fx);
        const float dy = -nf_div(nf_sub((float)h, cy_h), fy);
        const float dz = -1.0f;
        float* o = rd + p * 3;
        o[0] = nf_add(nf_add(nf_mul(dx, r00), nf_mul(dy, r01)), nf_mul(dz, r02));
        o[1] = nf_add(nf_add(nf_mul(dx, r10), nf_mul(dy, r11)), nf_mul(dz, r12));
        o[2] = nf_add(nf_add(nf_mul(dx, r20), nf_mul(dy, r21)), nf_mul(dz, r22));
        float* q = ro + p * 3;
        q[0] = t0; q[1] = t1; q[2] = t2;
    }
}

extern "C" int nf_ray_bundle(int height, int width, float fx, float fy, float cx_w, float cy_h, const float* c2w,
                             int c2w_row_stride, float* ro, float* rd, nf_stream_t stream) {
    if (height <= 0 || width <= 0 || !c2w || !ro || !rd || c2w_row_stride < 4) return NF_EINVAL;
    const int64_t n = (int64_t)height * width;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_ray_bundle, dim3(grid), dim3(256), 0, nf_s(stream), height, width, fx, fy, cx_w, cy_h, c2w,
                       c2w_row_stride, ro, rd);
    NF_RETURN_LAUNCH();
}

// K1 for a training batch: the rays of `n` selected pixels only (sel[i] = {row, col}, int64 as indexing hands them over, or flat
// pixel indices row * W + col as K0 / torch.multinomial return them), with the same arithmetic as k_ray_bundle -- bit-identical to gathering from the full bundle -- plus the
// gathers of the target pixels (image (H, W, C)) and of the background prior (H, W, 3) in the same pass.  Replaces the
// reference's full-frame get_ray_bundle + four index gathers per iteration (train_transformed_rays.py:302, 325-330).
__global__ void __launch_bounds__(256) k_ray_batch(int height, int width, float fx, float fy, float cx_w, float cy_h,
                                                   const float* __restrict__ c2w, int rs, const int64_t* __restrict__ sel, int flat, int64_t n,
                                                   const float* __restrict__ image, int channels, const float* __restrict__ bg,
                                                   float* __restrict__ ro, float* __restrict__ rd, float* __restrict__ target,
                                                   float* __restrict__ bg_out, int* __restrict__ bad) {
    const float r00 = c2w[0], r01 = c2w[1], r02 = c2w[2], t0 = c2w[3];
    const float r10 = c2w[rs + 0], r11 = c2w[rs + 1], r12 = c2w[rs + 2], t1 = c2w[rs + 3];
    const float r20 = c2w[2 * rs + 0], r21 = c2w[2 * rs + 1], r22 = c2w[2 * rs + 2], t2 = c2w[2 * rs + 3];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t h, w;
        if (flat) { const int64_t px = sel[i]; h = px >= 0 ? px / width : -1; w = px - h * width; }   // flat pixel index (what K0 returns)
        else { h = sel[2 * i]; w = sel[2 * i + 1]; }
        if (h < 0 || h >= height || w < 0 || w >= width) {            // reported to the host; the lane writes pixel (0, 0)
            atomicOr(bad, 1);
            h = 0; w = 0;
        }
        const float dx = nf_div(nf_sub((float)w, cx_w), fx);
        const float dy = -nf_div(nf_sub((float)h, cy_h), fy);
        const float dz = -1.0f;
        float* o = rd + i * 3;
        o[0] = nf_add(nf_add(nf_mul(dx, r00), nf_mul(dy, r01)), nf_mul(dz, r02));
        o[1] = nf_add(nf_add(nf_mul(dx, r10), nf_mul(dy, r11)), nf_mul(dz, r12));
        o[2] = nf_add(nf_add(nf_mul(dx, r20), nf_mul(dy, r21)), nf_mul(dz, r22));
        float* q = ro + i * 3;
        q[0] = t0; q[1] = t1; q[2] = t2;
        const int64_t pix = h * width + w;
        if (target)
            for (int c = 0; c < channels; ++c) target[i * channels + c] = image[pix * channels + c];
        if (bg_out)
            for (int c = 0; c < 3; ++c) bg_out[i * 3 + c] = bg[pix * 3 + c];
    }
}

extern "C" int nf_ray_batch(int height, int width, float fx, float fy, float cx_w, float cy_h, const float* c2w, int c2w_row_stride,
                            const int64_t* sel, int sel_is_flat, int64_t n, const float* image, int channels, const float* bg, float* ro,
                            float* rd, float* target, float* bg_out, int* bad_flag, nf_stream_t stream) {
    if (n == 0) return 0;
    if (height <= 0 || width <= 0 || n < 0 || !c2w || !sel || !ro || !rd || !bad_flag || c2w_row_stride < 4 ||
        (target && (!image || channels <= 0)) || (bg_out && !bg))
        return NF_EINVAL;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_ray_batch, dim3(grid), dim3(256), 0, nf_s(stream), height, width, fx, fy, cx_w, cy_h, c2w, c2w_row_stride,
                       sel, sel_is_flat ? 1 : 0, n, image, channels, bg, ro, rd, target, bg_out, bad_flag);
    NF_RETURN_LAUNCH();
}

// ---------------------------------------------------------------------------------------------
// K2: coarse depths (reference nerf/train_utils.py:56-76).
//   z = near*(1-t) + far*t with t = the caller's linspace(0,1,Nc) table;
//   perturb: z = lower + (upper-lower)*t_rand with mid-point brackets.  No FMA contraction.
// ---------------------------------------------------------------------------------------------
//   lindisp (T:65-66): z = 1 / (1/near * (1 - t) + 1/far * t), every operation a separately rounded fp32 one, in that order.
template <bool LINDISP>
__device__ __forceinline__ float nf_coarse_z(float t, float near_z, float far_z) {
    if (LINDISP) return nf_div(1.0f, nf_add(nf_mul(nf_div(1.0f, near_z), nf_sub(1.0f, t)), nf_mul(nf_div(1.0f, far_z), t)));
    return nf_add(nf_mul(near_z, nf_sub(1.0f, t)), nf_mul(far_z, t));
}

template <bool LINDISP>
__global__ void __launch_bounds__(256) k_sample_coarse(int64_t n_rays, int nc, float near_z, float far_z,
                                                       const float* __restrict__ t_vals,
                                                       const float* __restrict__ t_rand, float* __restrict__ z) {
    const int64_t total = n_rays * nc;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(p % nc);
        const float zi = nf_coarse_z<LINDISP>(t_vals[i], near_z, far_z);
        float out = zi;
        if (t_rand) {
            const float zl = i > 0 ? nf_coarse_z<LINDISP>(t_vals[i - 1], near_z, far_z) : zi;
            const float zu = i < nc - 1 ? nf_coarse_z<LINDISP>(t_vals[i + 1], near_z, far_z) : zi;
            const float lower = i > 0 ? nf_mul(0.5f, nf_add(zi, zl)) : zi;
            const float upper = i < nc - 1 ? nf_mul(0.5f, nf_add(zu, zi)) : zi;
            out = nf_add(lower, nf_mul(nf_sub(upper, lower), t_rand[p]));
        }
        z[p] = out;
    }
}

extern "C" int nf_sample_coarse_ex(int64_t n_rays, int n_coarse, float near_z, float far_z, const float* t_vals,
                                   const float* t_rand, int lindisp, float* z, nf_stream_t stream) {
    if (n_rays == 0) return 0;                       // nothing to do (empty tensors have NULL data pointers)
    if (n_rays < 0 || n_coarse <= 0 || !z || !t_vals) return NF_EINVAL;
    const int64_t total = n_rays * n_coarse;
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (lindisp)
        hipLaunchKernelGGL(k_sample_coarse<true>, dim3(grid), dim3(256), 0, nf_s(stream), n_rays, n_coarse, near_z, far_z, t_vals,
                           t_rand, z);
    else
        hipLaunchKernelGGL(k_sample_coarse<false>, dim3(grid), dim3(256), 0, nf_s(stream), n_rays, n_coarse, near_z, far_z, t_vals,
                           t_rand, z);
    NF_RETURN_LAUNCH();
}

extern "C" int nf_sample_coarse(int64_t n_rays, int n_coarse, float near_z, float far_z, const float* t_vals,
                                const float* t_rand, float* z, nf_stream_t stream) {
    return nf_sample_coarse_ex(n_rays, n_coarse, near_z, far_z, t_vals, t_rand, 0, z, stream);
}

// ---------------------------------------------------------------------------------------------
// K3: positional_encoding (reference nerf/nerf_helpers.py:195-239), stand-alone form (the hot path
// computes the encoding inside the fused MLP kernel; this entry point backs nerf.positional_encoding
// and the per-stage parity tests).  One thread per OUTPUT element so stores are fully coalesced.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_posenc(const float* __restrict__ x, int64_t n_rows, int dim, int n_freq,
                                                int include_input, float* __restrict__ out) {
    const int width = dim * (include_input + 2 * n_freq);
    const int64_t total = n_rows * width;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = p / width;
        int c = (int)(p - row * width);
        float v;
        if (include_input && c < dim) {
            v = x[row * dim + c];
        } else {
            c -= include_input ? dim : 0;
            const int blk = c / dim, comp = c - blk * dim;   // blk = 2*freq + (0: sin, 1: cos)
            const float a = nf_mul(x[row * dim + comp], exp2f((float)(blk >> 1)));
            v = (blk & 1) ? cosf(a) : sinf(a);
        }
        out[p] = v;
    }
}

extern "C" int nf_posenc(const float* x, int64_t n_rows, int dim, int n_freq, int include_input, float* out,
                         nf_stream_t stream) {
    if (n_rows == 0) return 0;
    if (n_rows < 0 || dim <= 0 || n_freq < 0 || n_freq > 30) return NF_EINVAL;
    const int64_t total = n_rows * dim * ((include_input ? 1 : 0) + 2 * n_freq);
    if (total == 0) return 0;                        // no frequencies and no input: an empty result (whose data pointer is NULL)
    if (!x || !out) return NF_EINVAL;
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(k_posenc, dim3(grid), dim3(256), 0, nf_s(stream), x, n_rows, dim, n_freq, include_input ? 1 : 0, out);
    NF_RETURN_LAUNCH();
}

// ---------------------------------------------------------------------------------------------
// Eval post-processing on the device (reference eval_transformed_rays.py): cast_to_image (EV:184-190: clamp to [0,1],
// x255, truncate to uint8 -- torchvision's ToPILImage does mul(255).byte()) and torch_normal_map (EV:84-119: back-project
// the "depth" map the script passes (it is disp_fine), cross product of forward differences, normalise, *0.5+0.5, blend
// towards white by the background weight, x255, truncate).  One thread per pixel; 16 B/pixel read, 6 B written.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void nf_backproject(const float* __restrict__ d, int r, int c, int width, float fx, float fy, float cx,
                                               float cy, float (&p)[3]) {
    const float dv = d[(int64_t)r * width + c];
    p[0] = nf_div(nf_mul(nf_sub((float)c, cx), dv), fx);
    p[1] = -nf_div(nf_mul(nf_sub((float)r, cy), dv), fy);
    p[2] = dv;
}

__global__ void __launch_bounds__(256) k_eval_postprocess(const float* __restrict__ rgb, const float* __restrict__ depth,
                                                          const float* __restrict__ weights, int height, int width, float fx, float fy,
                                                          float cx, float cy, uint8_t* __restrict__ rgb_u8,
                                                          uint8_t* __restrict__ normals_u8) {
    const int64_t n = (int64_t)height * width;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(q / width), c = (int)(q - (int64_t)r * width);
        if (rgb_u8) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float v = fminf(fmaxf(rgb[q * 3 + k], 0.0f), 1.0f);
                rgb_u8[q * 3 + k] = (uint8_t)nf_mul(v, 255.0f);
            }
        }
        if (normals_u8 && r < height - 1 && c < width - 1) {
            float p0[3], pr[3], pc[3];
            nf_backproject(depth, r, c, width, fx, fy, cx, cy, p0);
            nf_backproject(depth, r + 1, c, width, fx, fy, cx, cy, pr);          // dx: next row
            nf_backproject(depth, r, c + 1, width, fx, fy, cx, cy, pc);          // dy: next column
            const float ax = nf_sub(pc[0], p0[0]), ay = nf_sub(pc[1], p0[1]), az = nf_sub(pc[2], p0[2]);   // dy
            const float bx = nf_sub(pr[0], p0[0]), by = nf_sub(pr[1], p0[1]), bz = nf_sub(pr[2], p0[2]);   // dx
            // cross(dy, dx) as torch's CPU kernel rounds it: a1 * b2 - a2 * b1 = fma(a1, b2, -(a2 * b1)), the second product rounded, the
            // first exact inside the fused multiply-add (two rounded products differ from it by an ulp in a quarter of the components,
            // which moves about one byte in 40,000 of a normal map: nothing on the 48 x 48 and 64 x 64 fixtures, 37 bytes of 1030 x 1019)
            float nx = __fmaf_rn(ay, bz, -nf_mul(az, by));
            float ny = __fmaf_rn(az, bx, -nf_mul(ax, bz));
            float nz = __fmaf_rn(ax, by, -nf_mul(ay, bx));
            const float len = sqrtf(nf_add(nf_add(nf_mul(nx, nx), nf_mul(ny, ny)), nf_mul(nz, nz)));
            float v[3] = {nf_add(nf_mul(nf_div(nx, len), 0.5f), 0.5f), nf_add(nf_mul(nf_div(ny, len), 0.5f), 0.5f),
                          nf_add(nf_mul(nf_div(nz, len), 0.5f), 0.5f)};
            if (weights) {
                const float m = weights[q];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (m > 0.22f) v[k] = 1.0f;
                    v[k] = nf_add(nf_mul(nf_sub(1.0f, m), v[k]), m);
                }
            }
            uint8_t* o = normals_u8 + ((int64_t)r * (width - 1) + c) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = (uint8_t)(int)nf_mul(v[k], 255.0f);
        }
    }
}

extern "C" int nf_eval_postprocess(const float* rgb, const float* depthmap, const float* weights, int height, int width, float fx,
                                   float fy, float cx_w, float cy_h, uint8_t* rgb_u8, uint8_t* normals_u8, nf_stream_t stream) {
    if (height <= 0 || width <= 0 || (rgb_u8 && !rgb) || (normals_u8 && !depthmap)) return NF_EINVAL;
    const int64_t n = (int64_t)height * width;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_eval_postprocess, dim3(grid), dim3(256), 0, nf_s(stream), rgb, depthmap, weights, height, width, fx, fy,
                       cx_w, cy_h, rgb_u8, normals_u8);
    NF_RETURN_LAUNCH();
}
