// Exact-f32 inference forward of ConditionalBlendshapePaperNeRFModel that runs the colour layers only on samples the integrator can
// see: k_paper_mlp_fwd (nf_mlp.hip) with layers_dir.0 .. fc_rgb taken off the dead points.  A translation unit of its own: the
// objects of the other kernels do not change.
//
// A sample whose raw density is <= 0 has alpha = 1 - exp(-0 * dist) = 0 exactly, so the integrator multiplies its colour by an exact
// zero in every output; only the last sample of a ray (1e-6 is added to its density) and a NaN density keep their colour visible.
// Such a point is LIVE: !(sigma_raw <= 0) or p % S == S - 1.  Every other point is dead and gets rgb_raw = 0.
//
// Same persistent grid as k_paper_mlp_fwd (one workgroup per CU, four independent waves, 32 points per wave pass, no barrier), but no
// fixed share of the points per wave: the launch is cut into units of 32 consecutive points (unit u = points 32 u .. 32 u + 31), and a
// wave takes its next unit from a counter in device memory -- lane 0's atomicAdd, requested at the top of a pass for the pass after
// it, so that the round trip runs beside the trunk, and made a scalar with readfirstlane at the bottom.  How long a unit takes
// depends on whether its pass ends in a colour run, that is on where the object is; with fixed shares the launch ended with the
// wave whose share held the most runs (profiles/live_dynamic.md; tools/live_schedule_sim.py replays both orders).  A wave whose unit is
// past the end flushes its ring and leaves.  The counter is the library's (nf_live_counter, nf_mlp_live_kernel.h): one per stream,
// zeroed on the stream in front of every launch.  The kernel, its helpers and the launch stand in nf_mlp_live_kernel.h, shared
// with the instantiation that records what each wave did (nf_mlp_live_stats.hip).  A pass:
//   1. the trunk through fc_feat and fc_alpha alone (nf_paper_net_body<..., SIGMA>): feat of the 32 points in the wave's LDS slab,
//      sigma_raw in registers.  The pass has L live rows, D = 32 - L holes (dead or out-of-range points), and the wave's ring in
//      `scratch` (global memory) holds R rows from earlier passes, R <= 31;
//   2. R >= D: the D oldest ring rows move into the holes and layers_dir.0 .. fc_rgb run on the full slab.  The pass's own live rows
//      never leave the slab: they keep their place, their direction fragment and their sigma_raw in registers; a filled row takes
//      point index, direction fragment and sigma_raw from the ring.  (r, g, b, sigma_raw) go to `raw` by point index;
//   3. R < D (R + L <= 31): the L live rows are appended to the ring -- feat (1 KiB), the direction fragments (64 B), the point index
//      and sigma_raw -- and no colour layer runs.
// Dead points get (0, 0, 0, sigma_raw) in either case.  After its last unit a wave runs the colour layers on what the ring holds,
// moved into rows 0 .. R - 1 of the slab; the other rows hold whatever the slab held: MFMA columns are independent per point, and only
// the valid ones are stored.  Every point of `raw` is written exactly once.  An all-live pass touches no ring memory.
//
// A row moves with one wave-wide 16-byte access: lane l carries fragment l of the ring row (ds_read_b128 + one buffer store to append,
// one buffer load + ds_write_b128 to fill; the slab's swizzle is applied to the LDS address).  The colour run computes output tiles
// 0 .. 7 of layers_dir.0 only: tile 8 (fc_alpha) was computed by the trunk, and output tiles are independent MFMA chains.
//
// While fc_alpha's row runs alone over the 16 feat chunks the other accumulator tiles are dead: NfLivePre requests layers_dir.0's
// bias, first weight chunk and direction-chunk weights there, and the NF_LIVE_PF oldest ring rows, whether or not the pass will run
// the colour layers.
//
// Ring coherence.  Rows are written and read by the same wave, but by different lanes, and always in different passes.  In front of
// the first ring load of a pass (NfLivePre::wait, when fc_alpha's row starts) stands a workgroup-scope release / acquire fence pair
// around an explicit s_waitcnt vmcnt(0) (at workgroup scope the fences alone rely on the vector cache keeping one CU's accesses in
// order and emit no wait): every append has been acknowledged by L2 before a load is issued.  The ring loads carry sc1 (agent scope):
// they are served by that L2, where the write-through stores of this CU have landed, never by a line the per-CU vector cache kept from
// an earlier lap of the ring.  All ring traffic goes through a buffer descriptor that covers exactly the wave's ring: an index outside
// it is dropped by the range check, not written (NF_LIVE_OOB makes use of that for the lanes and rows that have nothing to move).
#include "nf_mlp_live_kernel.h"

extern "C" size_t nf_paper_mlp_fwd_live_scratch_floats(int max_workgroups) {
    return (size_t)nf_live_grid_cap(max_workgroups) * NF_MLP_WAVES * (NF_LIVE_WAVE_B / 4);
}

extern "C" int nf_paper_mlp_fwd_live(const float* packed, const float* cond, const float* ro, const float* rd, const float* rd_view,
                                     const float* z, int64_t n_rays, int n_samples, float* raw, float* scratch, size_t scratch_floats,
                                     int max_workgroups, nf_stream_t stream) {
    return nf_live_launch<false>(packed, cond, ro, rd, rd_view, z, n_rays, n_samples, raw, scratch, scratch_floats, max_workgroups, nullptr, stream);
}
