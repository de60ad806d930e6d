// k_inner_run.hip - the persistent run of the innermost level's 256 -> 256 layers (inner_run.hpp) behind two plain functions.
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

// workgroups of the run kernel one compute unit holds at once (0: the query failed - the run is then never selected)
int inner_run_workgroups_per_cu() {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)inner_run_kernel<kSameXcd>, 512, kInnerRunLds) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int launch_inner_run(const InnerRunArgs& ra, int B, hipStream_t st) {
    if (ra.n_layers < 1 || ra.n_layers > kInnerRunLayers || ra.nc != (B + 3) / 4) return fail(MPDX_E_INVALID, "inner run: %d layers, %d clusters for B=%d", ra.n_layers, ra.nc, B);
    hipLaunchKernelGGL(inner_run_kernel<kSameXcd>, dim3(inner_run_grid(B)), dim3(512), kInnerRunLds, st, ra);
    return 0;
}

}  // namespace mpdx
