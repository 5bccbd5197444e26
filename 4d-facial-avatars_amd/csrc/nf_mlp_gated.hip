// Exact-f32 inference forward of ConditionalBlendshapePaperNeRFModel that runs fc_feat, too, only where it is needed: the kernel of
// nf_mlp_live.hip (nf_mlp_live_kernel.h, GATE) with the trunk ended behind layers_xyz.5.  A translation unit of its own: the objects
// of the other kernels do not change.
//
// fc_feat has no activation, so in exact arithmetic sigma_raw = (a^T F) . h + (a . f + b), with h = relu(layers_xyz.5), (F, f) =
// fc_feat and (a, b) = fc_alpha.  For a dead sample (sigma_raw <= 0, not a ray's last) the integrator uses neither feat nor the
// colour, and sigma_raw only through relu(sigma_raw) = 0: fc_feat's 2,048 MFMAs per 32 points are spent to learn a sign.  The sign
// is proven here from a 256-term dot product on h and a rounding bound ("Sigma gate"):
//   w = a^T F, c = a . f + b            rounded to nearest from double
//   v = |a|^T |F|, d = |a| . |f| + |b|  rounded up from double
//   s = w . h + c,  u = v . h + d       rows 0 and 1 of ONE MFMA tile over h's 16 chunks, where fc_alpha's lone tile ran
//   proven dead  iff  s + 2^-13 u < -2^-100   (false for NaN or infinite operands; a ray's last sample is never proven)
// The kernel's own sigma_raw of a proven row would be <= s + 774 2^-24 u: no value that reaches an output is computed differently --
// the fold only picks rows whose colour and density the integrator multiplies by zero.
//
// A pass (the schedule, the ring, its fences, the unit counter: nf_mlp_live.hip, with "not proven" in place of "live"):
//   1. the trunk through layers_xyz.5 and the bound tile; the slab holds layers_xyz.5's accumulators as stored (ReLU on read);
//   2. the rows not proven stay in the slab or go to the ring exactly as live rows do, with their accumulators (the same 1 KiB), their
//      direction fragment, their point index and whether they are a ray's last sample (the meta row carries no density);
//   3. a gathered run is fc_feat, then layers_dir.0 in its nine-tile form (fc_alpha rides as tile 8), layers_dir.1, .2 and fc_rgb: the
//      MFMAs of k_paper_mlp_fwd from fc_feat on, in its order, so density and colour of a gathered row are k_paper_mlp_fwd's bit for
//      bit.  A gathered row that turns out dead (the bound could not prove it) is written with rgb 0 and its exact density, as
//      k_paper_mlp_fwd_live writes it;
//   4. a proven row is written as (0, 0, 0, s + 2^-13 u): negative, never NaN, and the only value that differs from the live kernel.
// While the bound tile runs alone, NfGatePre requests fc_feat's bias and first weight chunk and the oldest ring rows.
//
// The bound image (NF_BOUND_FLOATS floats): the tile's 16 chunks in packed fragment order ([ni][lane][4]: lane (g, i), r holds row i
// at k = 16 ni + 4 g + r; rows 2 .. 15 zero), then the tile's bias fragment (c, d, 0 ...).  k_paper_sigma_bound builds it from a packed
// image -- whoever packs builds it behind the pack; it is valid for exactly that image.
#include "nf_mlp_live_kernel.h"

// block ni: the 16 columns k = 16 ni .. + 15 of w and v.  Thread (part = tid >> 4, kk = tid & 15) sums rows n = 16 part .. + 15 in
// double; the 16 parts are added in order.  Block 0 also sums c and d.
__global__ void __launch_bounds__(256) k_paper_sigma_bound(const float* __restrict__ packed, float* __restrict__ bound) {
    using Net = NfPaperNet;
    __shared__ double sw[16][16], sv[16][16], sc[16], sd[16];
    __shared__ float fw[16], fv[16];
    const int tid = threadIdx.x, ni = blockIdx.x, part = tid >> 4, kk = tid & 15;
    // fc_alpha.weight[n]: tile 8 row 0 of layers_dir.0's chunk n / 16; fc_feat.weight[n][k]: block (k / 16, n / 16), lane (k / 4 % 4, n % 16)
    auto alpha = [&](int n) { return (double)packed[Net::OFF_D0 + (((n >> 4) * 9 + 8) * 64 + ((n >> 2) & 3) * 16) * 4 + (n & 3)]; };
    double w = 0.0, v = 0.0, c = 0.0, d = 0.0;
    for (int j = 0; j < 16; ++j) {
        const int n = 16 * part + j;
        const double a = alpha(n);
        const double f = (double)packed[Net::OFF_FEAT + ((ni * 16 + (n >> 4)) * 64 + (kk >> 2) * 16 + (n & 15)) * 4 + (kk & 3)];
        w += a * f;
        v += fabs(a) * fabs(f);
        if (ni == 0 && kk == 0) {
            const double b = (double)packed[Net::OFF_BIAS + Net::B_FEAT + n];
            c += a * b;
            d += fabs(a) * fabs(b);
        }
    }
    sw[part][kk] = w;
    sv[part][kk] = v;
    if (kk == 0) {
        sc[part] = c;
        sd[part] = d;
    }
    __syncthreads();
    // to nearest; up: the next f32 where the conversion came out below (NaN stays NaN, +inf stays)
    auto up = [](double x) {
        float f = (float)x;
        if ((double)f < x) f = nextafterf(f, INFINITY);
        return f;
    };
    if (tid < 16) {
        double tw = 0.0, tv = 0.0;
        for (int q = 0; q < 16; ++q) {
            tw += sw[q][tid];
            tv += sv[q][tid];
        }
        fw[tid] = (float)tw;
        fv[tid] = up(tv);
    }
    if (ni == 0 && tid == 16) {
        const double b = (double)packed[Net::OFF_BIAS + Net::B_D0 + 128];
        double tc = 0.0, td = 0.0;
        for (int q = 0; q < 16; ++q) {
            tc += sc[q];
            td += sd[q];
        }
        for (int j = 0; j < 16; ++j) bound[NF_BOUND_BIAS + j] = j == 0 ? (float)(tc + b) : (j == 1 ? up(td + fabs(b)) : 0.0f);
    }
    __syncthreads();
    const int lane = tid >> 2, r = tid & 3, g = lane >> 4, i = lane & 15;
    bound[(ni * 64 + lane) * 4 + r] = i == 0 ? fw[4 * g + r] : (i == 1 ? fv[4 * g + r] : 0.0f);
}

extern "C" size_t nf_paper_sigma_bound_floats(void) { return NF_BOUND_FLOATS; }

// bound: NF_BOUND_FLOATS floats, 16-byte aligned, for the image `packed` (nf_paper_pack)
extern "C" int nf_paper_sigma_bound(const float* packed, float* bound, nf_stream_t stream) {
    if (!packed || !bound || ((uintptr_t)bound & 15)) return NF_EINVAL;
    hipLaunchKernelGGL(k_paper_sigma_bound, dim3(16), dim3(256), 0, nf_s(stream), packed, bound);
    NF_RETURN_LAUNCH();
}

// nf_paper_mlp_fwd_live's arguments (the scratch is nf_paper_mlp_fwd_live_scratch_floats' too) and the bound image of `packed`
extern "C" int nf_paper_mlp_fwd_gated(const float* packed, const float* bound, const float* cond, const float* ro, const float* rd,
                                      const float* rd_view, const float* z, int64_t n_rays, int n_samples, float* raw, float* scratch,
                                      size_t scratch_floats, int max_workgroups, nf_stream_t stream) {
    return nf_live_launch<false, true>(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, scratch, scratch_floats, max_workgroups, nullptr,
                                       stream, bound);
}
