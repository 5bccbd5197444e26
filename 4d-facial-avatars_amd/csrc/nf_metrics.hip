// Image metrics of rendered frames against their test images, on the device: L1, MSE, PSNR and SSIM of N uint8 image pairs
// [N][H][W][3] in one launch -- what the reference's nerf/metrics.py (two_folders) takes from skimage's compare_psnr and
// compare_ssim(im1, im2, multichannel=True) on float images byte / 255, one frame at a time on the host.
//
// SSIM: 7 x 7 uniform window (NP = 49), sample covariance, averaged over the pixels whose whole window lies inside the image and over
// the channels.  Every window statistic of byte images is an exact integer, so the five sums (x, y, x^2, y^2, xy) are formed in int32
// and one float64 expression per pixel turns them into S:
//     K = 49 * 255, M = 48 * 49 * 255^2
//     ux = sx / K,  vx = (49 sxx - sx^2) / M,  vxy = (49 sxy - sx sy) / M
//     S  = ((2 sx sy + C1 K^2)(2 (49 sxy - sx sy) + C2 M)) / ((sx^2 + sy^2 + C1 K^2)((49 sxx - sx^2) + (49 syy - sy^2) + C2 M))
// (numerator and denominator of the textbook form multiplied by K^2 M; every integer term is exact in a double).
//
// The rows are interleaved RGB, so in byte columns j = 3 x + c a channel's horizontal window is the stride-3 sum of bytes
// j, j + 3, ..., j + 18: the kernel never separates the channels.  One workgroup takes a tile of 32 x 32 window origins (96 byte
// columns), i.e. 38 rows x 114 bytes of each image: bytes -> LDS, horizontal 7-sums of the five planes -> LDS (int32), vertical
// 7-sums + S per thread.  The same bytes give the tile's share of sum |a - b| and sum (a - b)^2 (each pixel owned by one tile).
// Reduction without floating-point atomics: per-tile partials in the workspace, the workgroup of an image that finishes last sums
// them in a fixed order (k_choice_level's ticket) and writes the image's results, so two runs are bit-identical.
#include "nf_common.h"

namespace nfm {
constexpr int TILE = 32;                   // window origins per tile side (pixels)
constexpr int HALO = 6;                    // 7-wide window: 6 more rows / pixels than origins
constexpr int ROWS = TILE + HALO;          // 38 input rows
constexpr int OUT_B = 3 * TILE;            // 96 byte columns of window origins
constexpr int IN_B = 3 * ROWS;             // 114 input byte columns
constexpr int IN_PITCH = 116;              // LDS row pitch of the byte tiles
constexpr int THREADS = 256;
constexpr int TICKET_ALIGN = 256;          // the tickets are a block of their own at the workspace's start (zeroed per call)
constexpr double K2 = 12495.0 * 12495.0;   // (49 * 255)^2
constexpr double M = 48.0 * 49.0 * 65025.0;
}  // namespace nfm

static inline int64_t nf_metrics_tiles(int extent) { return ((int64_t)extent - nfm::HALO + nfm::TILE - 1) / nfm::TILE; }
static inline size_t nf_metrics_ticket_bytes(int64_t n) {
    return (size_t)((n * 4 + nfm::TICKET_ALIGN - 1) / nfm::TICKET_ALIGN * nfm::TICKET_ALIGN);
}

extern "C" size_t nf_image_metrics_workspace_bytes(int64_t n, int height, int width) {
    if (n <= 0 || height < 7 || width < 7) return 0;
    return nf_metrics_ticket_bytes(n) + (size_t)n * (size_t)(nf_metrics_tiles(height) * nf_metrics_tiles(width)) * 3 * 8;
}

// fixed-order sum of one value per thread: lanes by xor-shuffle, then the four wave sums in index order
template <class T>
__device__ __forceinline__ T nf_metrics_block_sum(T v, T* s4) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                                   // s4 may still be read from the previous call
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

__global__ void __launch_bounds__(nfm::THREADS) k_image_metrics(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int height,
                                                                int width, int ntx, int nty, double c1k, double c2m,
                                                                unsigned* __restrict__ tickets, unsigned long long* __restrict__ partials,
                                                                double* __restrict__ out_f64, long long* __restrict__ out_i64) {
    using namespace nfm;
    __shared__ uint8_t s_a[ROWS][IN_PITCH], s_b[ROWS][IN_PITCH];
    __shared__ int s_h[5][ROWS][OUT_B];                                 // horizontal 7-sums of x, y, x^2, y^2, xy
    __shared__ unsigned long long s_u[4];
    __shared__ double s_d[4];
    __shared__ unsigned s_last;
    const int tid = threadIdx.x;
    const int tiles = ntx * nty;
    const int img = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int ty = tile / ntx, tx = tile % ntx;
    const int row0 = ty * TILE, col0 = tx * OUT_B;                      // first input row / byte column of the tile
    const int row_bytes = 3 * width;
    const size_t base = (size_t)img * height * row_bytes;

    // ---- bytes -> LDS (zeros outside the image); sum |d| and sum d^2 over the bytes this tile owns
    unsigned abs_sum = 0, sq_sum = 0;                                   // <= 17 bytes per thread: far inside 32 bits
    for (int i = tid; i < ROWS * IN_B; i += THREADS) {
        const int r = i / IN_B, c = i % IN_B;
        const int gy = row0 + r, gc = col0 + c;
        int va = 0, vb = 0;
        if (gy < height && gc < row_bytes) {
            const size_t at = base + (size_t)gy * row_bytes + gc;
            va = a[at];
            vb = b[at];
            if ((r < TILE || ty == nty - 1) && (c < OUT_B || tx == ntx - 1)) {
                const int d = va - vb;
                abs_sum += (unsigned)(d < 0 ? -d : d);
                sq_sum += (unsigned)(d * d);
            }
        }
        s_a[r][c] = (uint8_t)va;
        s_b[r][c] = (uint8_t)vb;
    }
    __syncthreads();

    // ---- horizontal 7-sums (stride 3 bytes = 1 pixel)
    for (int i = tid; i < ROWS * OUT_B; i += THREADS) {
        const int r = i / OUT_B, j = i % OUT_B;
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int x = s_a[r][j + 3 * k], y = s_b[r][j + 3 * k];
            sx += x;
            sy += y;
            sxx += x * x;
            syy += y * y;
            sxy += x * y;
        }
        s_h[0][r][j] = sx;
        s_h[1][r][j] = sy;
        s_h[2][r][j] = sxx;
        s_h[3][r][j] = syy;
        s_h[4][r][j] = sxy;
    }
    __syncthreads();

    // ---- vertical 7-sums and S per window origin, 12 origins per thread in a fixed order
    const int valid_rows = height - HALO - row0, valid_cols = 3 * (width - HALO) - col0;
    double ssim_sum = 0.0;
    for (int i = tid; i < TILE * OUT_B; i += THREADS) {
        const int r = i / OUT_B, j = i % OUT_B;
        if (r >= valid_rows || j >= valid_cols) continue;
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            sx += s_h[0][r + k][j];
            sy += s_h[1][r + k][j];
            sxx += s_h[2][r + k][j];
            syy += s_h[3][r + k][j];
            sxy += s_h[4][r + k][j];
        }
        // sx <= 12,495, sxx <= 3,186,225: 49 sxx <= 1.57e8, sx sy <= 1.57e8 -- all inside int32
        const int vx = 49 * sxx - sx * sx, vy = 49 * syy - sy * sy, vxy = 49 * sxy - sx * sy;
        const double n1 = (double)(2 * sx * sy) + c1k, n2 = (double)(2 * vxy) + c2m;
        const double d1 = (double)(sx * sx + sy * sy) + c1k, d2 = (double)(vx + vy) + c2m;
        ssim_sum += (n1 * n2) / (d1 * d2);
    }
    const unsigned long long abs_tile = nf_metrics_block_sum<unsigned long long>(abs_sum, s_u);
    const unsigned long long sq_tile = nf_metrics_block_sum<unsigned long long>(sq_sum, s_u);
    const double ssim_tile = nf_metrics_block_sum<double>(ssim_sum, s_d);

    // ---- partials -> workspace; the image's last workgroup reduces them
    unsigned long long* part = partials + ((size_t)img * tiles) * 3;
    if (tid == 0) {
        part[(size_t)tile * 3 + 0] = abs_tile;
        part[(size_t)tile * 3 + 1] = sq_tile;
        part[(size_t)tile * 3 + 2] = (unsigned long long)__double_as_longlong(ssim_tile);
        __threadfence();
        s_last = (atomicAdd(&tickets[img], 1u) == (unsigned)tiles - 1u) ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    unsigned long long abs_img = 0, sq_img = 0;
    double ssim_img = 0.0;
    for (int t = tid; t < tiles; t += THREADS) {                        // thread t: tiles t, t + 256, ... in index order
        abs_img += __hip_atomic_load(&part[(size_t)t * 3 + 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sq_img += __hip_atomic_load(&part[(size_t)t * 3 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ssim_img += __longlong_as_double((long long)__hip_atomic_load(&part[(size_t)t * 3 + 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    abs_img = nf_metrics_block_sum<unsigned long long>(abs_img, s_u);
    sq_img = nf_metrics_block_sum<unsigned long long>(sq_img, s_u);
    ssim_img = nf_metrics_block_sum<double>(ssim_img, s_d);
    if (tid == 0) {
        const double count = (double)height * (double)width * 3.0;
        const double mse = (double)sq_img / (65025.0 * count);
        out_f64[(size_t)img * 4 + 0] = (double)abs_img / (255.0 * count);
        out_f64[(size_t)img * 4 + 1] = mse;
        out_f64[(size_t)img * 4 + 2] = 10.0 * log10(1.0 / mse);          // +inf for identical images
        out_f64[(size_t)img * 4 + 3] = ssim_img / ((double)(height - HALO) * (double)(width - HALO) * 3.0);
        out_i64[(size_t)img * 2 + 0] = (long long)abs_img;
        out_i64[(size_t)img * 2 + 1] = (long long)sq_img;
    }
}

extern "C" int nf_image_metrics(const uint8_t* a, const uint8_t* b, int64_t n, int height, int width, double ssim_range, void* workspace,
                                size_t workspace_bytes, double* out_f64, int64_t* out_i64, nf_stream_t stream) {
    if (n < 0 || height < 7 || width < 7) return NF_EINVAL;
    if (n == 0) return 0;                                               // (empty tensors have NULL data pointers)
    if (!a || !b || !workspace || !out_f64 || !out_i64) return NF_EINVAL;
    if (workspace_bytes < nf_image_metrics_workspace_bytes(n, height, width)) return NF_EINVAL;
    const int64_t ntx = nf_metrics_tiles(width), nty = nf_metrics_tiles(height);
    if ((int64_t)width * 3 > 0x7fffffff || ntx * nty > 0x7fffffff || n * ntx * nty > 0x7fffffff) return NF_EINVAL;
    const size_t ticket_bytes = nf_metrics_ticket_bytes(n);
    hipError_t e = hipMemsetAsync(workspace, 0, ticket_bytes, nf_s(stream));
    if (e != hipSuccess) return (int)e;
    const double c1 = (0.01 * ssim_range) * (0.01 * ssim_range), c2 = (0.03 * ssim_range) * (0.03 * ssim_range);
    hipLaunchKernelGGL(k_image_metrics, dim3((unsigned)(n * ntx * nty)), dim3(nfm::THREADS), 0, nf_s(stream), a, b, height, width, (int)ntx,
                       (int)nty, c1 * nfm::K2, c2 * nfm::M, reinterpret_cast<unsigned*>(workspace),
                       reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + ticket_bytes), out_f64,
                       reinterpret_cast<long long*>(out_i64));
    NF_RETURN_LAUNCH();
}
