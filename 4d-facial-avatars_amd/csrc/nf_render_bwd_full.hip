// K5 full backward: d_raw (and d_bg) from a cotangent of EVERY output of the volume integrator -- rgb, the third output (disparity in
// NeRFace mode, depth map in tiny mode), acc, the weights, and weights[:, -1] on its own.  k_volume_render_bwd (nf_render.hip) stays
// the path of a backward that carries d_rgb only; this kernel is the same two passes with the other cotangents folded into dL/dw.
//
// With b_j = 1-alpha_j+1e-10, T_i = prod_{j<i} b_j, w_i = alpha_i T_i, A = sum w_i, D = sum w_i z_i, q = D / A:
//   dL/dw_i = <d_rgb, c_i> (+ white-bg term: -sum(d_rgb)) + d_acc + d_weights[i] + [i == S-1] d_w_last + d_third * t_i
//     NeRFace mode: third = 1 / max(1e-10, q) (V:69), t_i = -third^2 (z_i - q) / A  if q > 1e-10, else 0
//     tiny mode:    third = D,                        t_i = z_i
//   dL/dalpha_i, dL/dsigma_i, the ReLU mask and dL/draw_rgb: as in k_volume_render_bwd (the suffix sum taken from the far end)
//   dL/dbg = w_{S-1} d_rgb   (the last sample's colour IS the background prior, Quirk Q5)
// Difference from the reference, on purpose: a ray with A == 0 has q = 0/0 = NaN.  (NeRFace mode's last sample has dist 1e10 |rd|
// and sigma >= 1e-6, so alpha_{S-1} = 1 and A > 0 for any |rd| a camera produces; A == 0 needs |rd| below ~1e-12.)  The
// reference's torch.max(1e-10, q) propagates the NaN into the disparity and so into every gradient of the ray; the forward kernel's
// fmaxf returns 1e-10 there (disparity 1e10), and this backward is the derivative of THAT forward: the constant branch, a zero
// disparity gradient.  DESIGN section 7 lists it.
// A and D are needed before any dL/dw: one more pair of wave reductions between the two passes.  Mapping as everywhere in K5: one
// wavefront per ray, sample s in lane s % 64 of chunk s / 64, forward quantities recomputed in registers, no LDS.
#include "nf_render_dev.h"

template <int NCH>
__global__ void __launch_bounds__(256) k_volume_render_bwd_full(const float* __restrict__ raw, const float* __restrict__ z,
                                                                const float* __restrict__ rd, const float* __restrict__ noise,
                                                                const float* __restrict__ bg, const float* __restrict__ d_rgb,
                                                                const float* __restrict__ d_third, const float* __restrict__ d_acc,
                                                                const float* __restrict__ d_weights, const float* __restrict__ d_w_last,
                                                                int64_t n_rays, int S, int white_bg, float* __restrict__ d_raw,
                                                                float* __restrict__ d_bg, int mode) {
    const int lane = nf_lane();
    const int64_t ray = (int64_t)blockIdx.x * NF_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const float4* raw_row = reinterpret_cast<const float4*>(raw) + ray * S;
    const float* z_row = z + ray * S;
    const float* noise_row = noise ? noise + ray * S : nullptr;
    const float* bg_ray = bg ? bg + ray * 3 : nullptr;
    const float* gw_row = d_weights ? d_weights + ray * S : nullptr;
    const float norm = (mode & 1) ? nf_rd_norm(rd + ray * 3) : 1.0f;
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    if (d_rgb) { g0 = d_rgb[ray * 3 + 0]; g1 = d_rgb[ray * 3 + 1]; g2 = d_rgb[ray * 3 + 2]; }
    const float gw_white = white_bg ? -(g0 + g1 + g2) : 0.0f;
    const float g_acc = d_acc ? d_acc[ray] : 0.0f;
    const float g_third = d_third ? d_third[ray] : 0.0f;
    const float g_last = d_w_last ? d_w_last[ray] : 0.0f;

    float T[NCH], w[NCH], dw[NCH], alpha[NCH], dist[NCH], pre[NCH], zz[NCH], c[NCH][3];
    float carry = 1.0f;
    float a_w = 0.0f, a_d = 0.0f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int s = k * 64 + lane;
        const bool on = s < S;
        alpha[k] = 0.f; dist[k] = 0.f; pre[k] = 0.f; zz[k] = 0.f; c[k][0] = c[k][1] = c[k][2] = 0.f;
        float gws = 0.0f;                      // the cotangents that reach w_s directly
        if (on) {
            const NfSample q = nf_load_sample(raw_row, z_row, noise_row, bg_ray, norm, s, S, mode);
            alpha[k] = q.alpha; dist[k] = q.dist; pre[k] = q.pre;
            c[k][0] = q.c[0]; c[k][1] = q.c[1]; c[k][2] = q.c[2];
            zz[k] = z_row[s];
            gws = g_acc;
            if (gw_row) gws += gw_row[s];
            if (s == S - 1) gws += g_last;
        }
        const float b = on ? nf_add(nf_sub(1.0f, alpha[k]), 1e-10f) : 1.0f;
        const float incl = wave_scan_mul(b);
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0f;
        T[k] = carry * excl;
        w[k] = alpha[k] * T[k];
        dw[k] = on ? (g0 * c[k][0] + g1 * c[k][1] + g2 * c[k][2] + gw_white) + gws : 0.0f;
        a_w += w[k]; a_d += w[k] * zz[k];
        carry *= __shfl(incl, 63, 64);
    }
    if (d_third) {                             // wave-uniform
        const float A = wave_sum(a_w), D = wave_sum(a_d);
        if (mode & 4) {
#pragma unroll
            for (int k = 0; k < NCH; ++k) if (k * 64 + lane < S) dw[k] += g_third * zz[k];
        } else {
            const float q = D / A;
            if (q > 1e-10f) {                  // else the max() of V:69 passes the constant: no gradient (a NaN q lands here too)
                const float disp = 1.0f / q;
                const float coef = -(g_third * disp * disp) / A;
#pragma unroll
                for (int k = 0; k < NCH; ++k) if (k * 64 + lane < S) dw[k] += coef * (zz[k] - q);
            }
        }
    }
    // sum_{j>s} dw_j w_j from the far end, over the terms behind s only (see k_volume_render_bwd)
    float after = 0.0f;                        // sum over all later chunks of dw*w
#pragma unroll
    for (int k = NCH - 1; k >= 0; --k) {
        const int s = k * 64 + lane;
        const float rincl = wave_rscan_add(dw[k] * w[k]);
        float rexcl = __shfl_down(rincl, 1, 64);
        if (lane == 63) rexcl = 0.0f;
        const float suffix = after + rexcl;
        after += __shfl(rincl, 0, 64);
        if (s < S) {
            const float b = (1.0f - alpha[k]) + 1e-10f;
            const float d_alpha = dw[k] * T[k] - suffix / b;
            const float d_sigma = d_alpha * dist[k] * (1.0f - alpha[k]);
            float4 o;
            if (bg_ray && s == S - 1) {          // the background sample: its colour is the prior, not raw
                o.x = o.y = o.z = 0.0f;
                if (d_bg) { d_bg[ray * 3 + 0] = w[k] * g0; d_bg[ray * 3 + 1] = w[k] * g1; d_bg[ray * 3 + 2] = w[k] * g2; }
            } else {
                o.x = w[k] * g0 * c[k][0] * (1.0f - c[k][0]);
                o.y = w[k] * g1 * c[k][1] * (1.0f - c[k][1]);
                o.z = w[k] * g2 * c[k][2] * (1.0f - c[k][2]);
            }
            o.w = pre[k] > 0.0f ? d_sigma : 0.0f;
            reinterpret_cast<float4*>(d_raw)[ray * S + s] = o;
        }
    }
}

static int nf_volume_render_bwd_full_impl(const float* raw, const float* z, const float* rd, const float* noise, const float* bg,
                                          const float* d_rgb, const float* d_third, const float* d_acc, const float* d_weights,
                                          const float* d_w_last, int64_t n_rays, int n_samples, int white_background, float* d_raw,
                                          float* d_bg, int mode, nf_stream_t stream) {
    if (n_rays == 0) return 0;                       // nothing to do (empty tensors have NULL data pointers)
    if (!raw || !z || (!rd && (mode & 1)) || !d_raw || n_rays < 0 || n_samples <= 0 || n_samples > 64 * NF_MAX_CHUNKS) return NF_EINVAL;
    if (!d_rgb && !d_third && !d_acc && !d_weights && !d_w_last) return NF_EINVAL;     // no cotangent at all: nothing to differentiate
    if (d_bg && !bg) return NF_EINVAL;               // d_bg is the gradient of the prior: there has to be one
    const int64_t grid = (n_rays + NF_RAYS_PER_BLOCK - 1) / NF_RAYS_PER_BLOCK;
    if (grid > 0x7fffffff) return NF_EINVAL;
    const int nch = (n_samples + 63) / 64;
#define NF_BWD_FULL(N)                                                                                                        \
    hipLaunchKernelGGL(k_volume_render_bwd_full<N>, dim3((unsigned)grid), dim3(256), 0, nf_s(stream), raw, z, rd, noise, bg,  \
                       d_rgb, d_third, d_acc, d_weights, d_w_last, n_rays, n_samples, white_background, d_raw, d_bg, mode)
    if (nch == 1) NF_BWD_FULL(1); else if (nch == 2) NF_BWD_FULL(2); else if (nch == 3) NF_BWD_FULL(3); else if (nch == 4) NF_BWD_FULL(4);
    else if (nch <= 8) NF_BWD_FULL(8); else NF_BWD_FULL(16);
#undef NF_BWD_FULL
    NF_RETURN_LAUNCH();
}

extern "C" int nf_volume_render_bwd_full(const float* raw, const float* z, const float* rd, const float* noise, const float* bg,
                                         const float* d_rgb, const float* d_disp, const float* d_acc, const float* d_weights,
                                         const float* d_w_last, int64_t n_rays, int n_samples, int white_background, float* d_raw,
                                         float* d_bg, nf_stream_t stream) {
    return nf_volume_render_bwd_full_impl(raw, z, rd, noise, bg, d_rgb, d_disp, d_acc, d_weights, d_w_last, n_rays, n_samples,
                                          white_background, d_raw, d_bg, NF_VR_NERFACE, stream);
}

// tiny_nerf's render_volume_density (tiny_nerf.py:68-107) through all three of its outputs: (rgb_map, depth_map, acc_map).
extern "C" int nf_render_volume_density_bwd_full(const float* raw, const float* depth, const float* d_rgb, const float* d_depth,
                                                 const float* d_acc, int64_t n_rays, int n_samples, float* d_raw, nf_stream_t stream) {
    return nf_volume_render_bwd_full_impl(raw, depth, nullptr, nullptr, nullptr, d_rgb, d_depth, d_acc, nullptr, nullptr, n_rays,
                                          n_samples, 0, d_raw, nullptr, NF_VR_TINY, stream);
}
