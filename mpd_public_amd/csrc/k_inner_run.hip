// k_inner_run.hip - the persistent runs of inner-level layers (inner_run.hpp: the seven 256 -> 256 layers, the tail of up level 0) behind plain functions.
#include "host.hpp"
#include "inner_run.hpp"

namespace mpdx {

// Placement of a cluster's 8 workgroups (inner_run.hpp): 1 = on one XCD, 0 = spread over the 8 XCDs.  A compile-time choice; results do not depend on it.
// Measured (profiles/inner_run_ab.md, cfg 2, ms per plan): per-layer launches 17.59, cluster spread 17.07, cluster on one XCD 16.75 - kept.
#ifndef MPDX_INNER_RUN_SAME_XCD
#define MPDX_INNER_RUN_SAME_XCD 1
#endif
static constexpr bool kSameXcd = MPDX_INNER_RUN_SAME_XCD != 0;

bool inner_run_width_ok(int width) { return width == kRunWide || width == kRunNarrow; }
int inner_run_clusters(int B, int width) { return inner_run_width_ok(width) ? run_clusters(B, width) : 0; }
int inner_run_grid(int B, int width) { return run_grid(inner_run_clusters(B, width), kSameXcd); }
void inner_run_slot(int block, int* cluster, int* tile) { const RunSlot s = run_slot(block, kSameXcd); *cluster = s.c; *tile = s.m; }

template <class SEQ>
static int workgroups_per_cu() {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)inner_run_kernel<SEQ, kSameXcd>, 512, SEQ::lds()) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}
// workgroups of a run kernel one compute unit holds at once (0: the query failed, or no such width - that run is then never selected)
int inner_run_workgroups_per_cu(int width) {
    return width == kRunWide ? workgroups_per_cu<RunSeqSeven<kRunWide>>() : width == kRunNarrow ? workgroups_per_cu<RunSeqSeven<kRunNarrow>>() : 0;
}
int tail_run_workgroups_per_cu(int width) {
    return width == kRunWide ? workgroups_per_cu<RunSeqTail<kRunWide>>() : width == kRunNarrow ? workgroups_per_cu<RunSeqTail<kRunNarrow>>() : 0;
}

template <class SEQ>
static int launch_run(const typename SEQ::Args& ra, int B, hipStream_t st, const char* what) {
    if (ra.n_layers != SEQ::kLayers || ra.nc != run_clusters(B, SEQ::kWidth))
        return fail(MPDX_E_INVALID, "%s: %d layers, %d clusters for B=%d at width %d", what, ra.n_layers, ra.nc, B, SEQ::kWidth);
    hipLaunchKernelGGL((inner_run_kernel<SEQ, kSameXcd>), dim3(run_grid(ra.nc, kSameXcd)), dim3(512), SEQ::lds(), st, ra);
    return 0;
}
int launch_inner_run(const InnerRunArgs& ra, int B, int width, hipStream_t st) {
    if (width == kRunNarrow) return launch_run<RunSeqSeven<kRunNarrow>>(ra, B, st, "inner run");
    if (width == kRunWide) return launch_run<RunSeqSeven<kRunWide>>(ra, B, st, "inner run");
    return fail(MPDX_E_INVALID, "inner run: width %d", width);
}
int launch_tail_run(const TailRunArgs& ra, int B, int width, hipStream_t st) {
    if (width == kRunNarrow) return launch_run<RunSeqTail<kRunNarrow>>(ra, B, st, "tail run");
    if (width == kRunWide) return launch_run<RunSeqTail<kRunWide>>(ra, B, st, "tail run");
    return fail(MPDX_E_INVALID, "tail run: width %d", width);
}

}  // namespace mpdx
