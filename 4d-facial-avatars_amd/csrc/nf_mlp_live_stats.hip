// k_paper_mlp_fwd_live<., STATS> (nf_mlp_live_kernel.h): the kernel of nf_mlp_live.hip with a per-wave record of what the wave did --
// units taken, colour runs, rows of the final flush, the wall clock at exit and, on request, the shader clocks of a pass's phases
// (nf_live_mark).  An instrument for the tests of the dynamic schedule, for profiles/live_dynamic.md and profiles/sigma_gate_fine.md; no render path calls it.  A translation unit of its own: the production kernel's object does not
// depend on it.
#include "nf_mlp_live_kernel.h"

static int nf_live_stats_launch(bool clocks, const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                const float* z, int64_t n_rays, int n_samples, float* raw, float* scratch, size_t scratch_floats,
                                int max_workgroups, int64_t* stats, size_t stats_rows, nf_stream_t stream) {
    static_assert(sizeof(long long) == sizeof(int64_t), "a statistics row is int64s");
    if (max_workgroups < 0 || !stats || ((uintptr_t)stats & 7) || stats_rows < (size_t)nf_live_grid_cap(max_workgroups) * NF_MLP_WAVES) return NF_EINVAL;
    const size_t cols = NF_LIVE_STAT_COLS + (clocks ? NF_LIVE_PHASES : 0);
    const hipError_t e = hipMemsetAsync(stats, 0, stats_rows * cols * sizeof(int64_t), nf_s(stream));
    if (e != hipSuccess) return (int)e;
    return nf_live_launch<true>(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, scratch, scratch_floats, max_workgroups,
                                reinterpret_cast<long long*>(stats), stream, nullptr, clocks);
}

extern "C" int nf_paper_mlp_fwd_live_stats(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                           const float* z, int64_t n_rays, int n_samples, float* raw, float* scratch, size_t scratch_floats,
                                           int max_workgroups, int64_t* stats, size_t stats_rows, nf_stream_t stream) {
    return nf_live_stats_launch(false, packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, scratch, scratch_floats, max_workgroups, stats,
                                stats_rows, stream);
}

// rows of NF_LIVE_STAT_COLS + NF_LIVE_PHASES: the clocks of a pass's phases behind the four columns
extern "C" int nf_paper_mlp_fwd_live_phases(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                            const float* z, int64_t n_rays, int n_samples, float* raw, float* scratch, size_t scratch_floats,
                                            int max_workgroups, int64_t* stats, size_t stats_rows, nf_stream_t stream) {
    return nf_live_stats_launch(true, packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, scratch, scratch_floats, max_workgroups, stats,
                                stats_rows, stream);
}
