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

int inner_run_grid(int B) {
    const int nc = (B + 3) / 4;
    return kSameXcd ? ((nc + 7) / 8) * 64 : nc * 8;
}

template <class SEQ>
static int workgroups_per_cu() {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)inner_run_kernel<SEQ, kSameXcd>, 512, SEQ::lds()) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}
// workgroups of a run kernel one compute unit holds at once (0: the query failed - that run is then never selected)
int inner_run_workgroups_per_cu() { return workgroups_per_cu<RunSeqSeven>(); }
int tail_run_workgroups_per_cu() { return workgroups_per_cu<RunSeqTail>(); }

template <class SEQ>
static int launch_run(const typename SEQ::Args& ra, int B, hipStream_t st, const char* what) {
    if (ra.n_layers != SEQ::kLayers || ra.nc != (B + 3) / 4) return fail(MPDX_E_INVALID, "%s: %d layers, %d clusters for B=%d", what, ra.n_layers, ra.nc, B);
    hipLaunchKernelGGL((inner_run_kernel<SEQ, kSameXcd>), dim3(inner_run_grid(B)), dim3(512), SEQ::lds(), st, ra);
    return 0;
}
int launch_inner_run(const InnerRunArgs& ra, int B, hipStream_t st) { return launch_run<RunSeqSeven>(ra, B, st, "inner run"); }
int launch_tail_run(const TailRunArgs& ra, int B, hipStream_t st) { return launch_run<RunSeqTail>(ra, B, st, "tail run"); }

}  // namespace mpdx
