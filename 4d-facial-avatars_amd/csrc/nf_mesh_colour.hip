// Per-vertex radiance of a mesh: the short ray through the surface at every vertex, and the composite of the network's output along
// it (DESIGN.md "Mesh colours" is the normative text; tests/mesh_colour_ref.py restates it in NumPy).
//
//   rays       vertex v, normal n (towards lower density), K samples, half-thickness `depth`:
//                rd = -n (a sign flip; the origin of the ray is v itself, so none is written)
//                z[k] = float(2 k - K + 1) * half, half = depth / float(K): from outside (z < 0) to inside, spacing 2 half; the
//                middle sample of an odd K is the vertex exactly
//                rd_view, with a camera-to-world [R | o]: t = v - o, d = -((t0 R02 + t1 R12) + t2 R22) (minus the vertex's z in the
//                camera frame); d > 0: t / d, the un-normalised direction of the pixel that sees v (no intrinsics in it); otherwise
//                (behind the camera, on its plane, or d not a number) the central ray (-R02, -R12, -R22).  Without a camera:
//                (0, 0, view_z) for every vertex.
//              Every operation rounded on its own, in the association written: NumPy float32 gives the same bits.
//   integrate  raw[V][K][4], step h, per vertex over k ascending: sigma = relu(raw[k][3]) (a NaN stays), alpha = 1 - expf(-sigma h),
//              T_k = prod_{j<k} (1 - alpha_j), w = alpha T, opacity = sum w, c = sum w sigmoid(raw[k][:3]); the colour is c / opacity
//              where opacity >= min_opacity, else sigmoid(raw[K / 2][:3]).  No background sample, no 1e-10 at the far end, no
//              scaling by |rd|, nothing added to a density.
//
// k_mcol_rays: one thread per entry of z (V K of them, at least V); the first V threads also do their vertex.  k_mcol_integrate: one
// thread per vertex, 256 per workgroup.  A vertex's K samples are K x 16 contiguous bytes and the vertices of a wave lie one behind
// the other, so the workgroup fetches CHUNK samples of its 256 vertices at a time with loads in which CHUNK adjacent lanes cover
// one vertex's run (K = CHUNK: 1 KiB per wave and load, unbroken) into LDS, and every thread then walks its own row there, in
// ascending k: one fixed order per vertex, no float atomics, the same bits from run to run.
#include <math.h>
#include "nf_scan_dev.h"
#include "nf_render_dev.h"

namespace nfk {
constexpr int MAX_SAMPLES = 64;            // K of either entry point
constexpr int CHUNK = 8;                   // samples per vertex and round of k_mcol_integrate: 128 B, one cache line
constexpr int ROW = CHUNK + 1;             // float4 per vertex in LDS: 144 B apart, so that the threads' 16-byte reads spread over the banks
}  // namespace nfk

__global__ void __launch_bounds__(nfc::THREADS) k_mcol_rays(const float* __restrict__ vertices, const float* __restrict__ normals, int64_t n_vertices,
                                                            const float* __restrict__ c2w, int64_t stride, float view_z, int n_samples, float depth,
                                                            float* __restrict__ rd, float* __restrict__ rd_view, float* __restrict__ z) {
    const int64_t base = (int64_t)blockIdx.x * nfc::THREADS, i = base + threadIdx.x;
    if (i >= n_vertices * n_samples) return;
    const int k = (int)(((uint32_t)(base % n_samples) + threadIdx.x) % (uint32_t)n_samples);       // the 64-bit remainder once per workgroup
    z[i] = nf_mul((float)(2 * k - n_samples + 1), nf_div(depth, (float)n_samples));
    if (i >= n_vertices) return;
    rd[i * 3 + 0] = -normals[i * 3 + 0], rd[i * 3 + 1] = -normals[i * 3 + 1], rd[i * 3 + 2] = -normals[i * 3 + 2];
    float vx = 0.f, vy = 0.f, vz = view_z;
    if (c2w) {
        const float r02 = c2w[2], r12 = c2w[stride + 2], r22 = c2w[2 * stride + 2];
        const float t0 = nf_sub(vertices[i * 3 + 0], c2w[3]), t1 = nf_sub(vertices[i * 3 + 1], c2w[stride + 3]);
        const float t2 = nf_sub(vertices[i * 3 + 2], c2w[2 * stride + 3]);
        const float d = -nf_add(nf_add(nf_mul(t0, r02), nf_mul(t1, r12)), nf_mul(t2, r22));
        const bool front = d > 0.f;                                     // false for a NaN
        vx = front ? nf_div(t0, d) : -r02;
        vy = front ? nf_div(t1, d) : -r12;
        vz = front ? nf_div(t2, d) : -r22;
    }
    rd_view[i * 3 + 0] = vx, rd_view[i * 3 + 1] = vy, rd_view[i * 3 + 2] = vz;
}

__global__ void __launch_bounds__(nfc::THREADS) k_mcol_integrate(const float4* __restrict__ raw, int64_t n_vertices, int n_samples, float step,
                                                                 float min_opacity, float* __restrict__ colour, float* __restrict__ opacity) {
    __shared__ float4 s_raw[nfc::THREADS * nfk::ROW];
    const int64_t v0 = (int64_t)blockIdx.x * nfc::THREADS, v = v0 + threadIdx.x;
    const int middle = n_samples / 2;
    float trans = 1.f, acc = 0.f, cr = 0.f, cg = 0.f, cb = 0.f, mr = 0.f, mg = 0.f, mb = 0.f;
    for (int k0 = 0; k0 < n_samples; k0 += nfk::CHUNK) {                // the same trips in every thread: the barriers are the workgroup's
        __syncthreads();                                                // the round before has been read
#pragma unroll
        for (int j = 0; j < nfk::CHUNK; ++j) {
            const int e = j * nfc::THREADS + threadIdx.x, row = e / nfk::CHUNK, s = k0 + e % nfk::CHUNK;
            if (v0 + row < n_vertices && s < n_samples) s_raw[row * nfk::ROW + e % nfk::CHUNK] = raw[(v0 + row) * n_samples + s];
        }
        __syncthreads();
        if (v >= n_vertices) continue;
        const int n = n_samples - k0 < nfk::CHUNK ? n_samples - k0 : nfk::CHUNK;
        for (int q = 0; q < n; ++q) {
            const float4 r = s_raw[threadIdx.x * nfk::ROW + q];
            const float sr = nf_sigmoid(r.x), sg = nf_sigmoid(r.y), sb = nf_sigmoid(r.z);
            if (k0 + q == middle) mr = sr, mg = sg, mb = sb;
            const float sigma = r.w < 0.f ? 0.f : r.w;                  // torch.relu: a NaN stays a NaN
            const float alpha = nf_sub(1.f, expf(-nf_mul(sigma, step)));
            const float w = nf_mul(alpha, trans);
            acc = nf_add(acc, w);
            cr = nf_add(cr, nf_mul(w, sr)), cg = nf_add(cg, nf_mul(w, sg)), cb = nf_add(cb, nf_mul(w, sb));
            trans = nf_mul(trans, nf_sub(1.f, alpha));
        }
    }
    if (v >= n_vertices) return;
    const bool seen = acc >= min_opacity;                               // false for a NaN
    colour[v * 3 + 0] = seen ? nf_div(cr, acc) : mr;
    colour[v * 3 + 1] = seen ? nf_div(cg, acc) : mg;
    colour[v * 3 + 2] = seen ? nf_div(cb, acc) : mb;
    opacity[v] = acc;
}

// ---- entry points
extern "C" int nf_mesh_colour_rays(const float* vertices, const float* normals, int64_t n_vertices, const float* c2w, int64_t c2w_row_stride,
                                   float view_z, int n_samples, float depth, float* rd, float* rd_view, float* z, nf_stream_t stream) {
    if (n_vertices < 0 || n_vertices > 0x7fffffff || n_samples < 1 || n_samples > nfk::MAX_SAMPLES || !(depth >= 0.f)) return NF_EINVAL;   // NaN fails
    if (c2w && c2w_row_stride < 4) return NF_EINVAL;
    if (!n_vertices) return 0;
    if (!vertices || !normals || !rd || !rd_view || !z) return NF_EINVAL;
    hipLaunchKernelGGL(k_mcol_rays, dim3((unsigned)nf_blocks(n_vertices * n_samples)), dim3(nfc::THREADS), 0, nf_s(stream), vertices, normals, n_vertices,
                       c2w, c2w_row_stride, view_z, n_samples, depth, rd, rd_view, z);
    NF_RETURN_LAUNCH();
}

extern "C" int nf_mesh_colour_integrate(const float* raw, int64_t n_vertices, int n_samples, float step, float min_opacity, float* colour,
                                        float* opacity, nf_stream_t stream) {
    if (n_vertices < 0 || n_vertices > 0x7fffffff || n_samples < 1 || n_samples > nfk::MAX_SAMPLES) return NF_EINVAL;
    if (!(step >= 0.f) || min_opacity != min_opacity) return NF_EINVAL;
    if (!n_vertices) return 0;
    if (!raw || !colour || !opacity || (reinterpret_cast<uintptr_t>(raw) & 15)) return NF_EINVAL;      // the samples are read 16 bytes at a time
    hipLaunchKernelGGL(k_mcol_integrate, dim3((unsigned)nf_blocks(n_vertices)), dim3(nfc::THREADS), 0, nf_s(stream), reinterpret_cast<const float4*>(raw),
                       n_vertices, n_samples, step, min_opacity, colour, opacity);
    NF_RETURN_LAUNCH();
}
