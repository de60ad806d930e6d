// k_chain.hip - the guide and trajectory-metrics kernels of a table-driven serial chain (chain.hpp): every instantiation (1 ... 8 joints, one scene
// or several) behind two launchers; k_guide.hip checks the block and dispatches here.
#include "host.hpp"
#include "chain.hpp"

namespace mpdx {

template <int QD>
static int chain_guide_qd(const ChainGuideArgs& ca, bool multi, size_t lds, int B, hipStream_t st) {
    if (multi) {
        if (int rc = raise_lds_limit((const void*)guide_step_chain_kernel<QD, true>)) return rc;
        hipLaunchKernelGGL((guide_step_chain_kernel<QD, true>), dim3(B), dim3(512), lds, st, ca);
    } else {
        if (int rc = raise_lds_limit((const void*)guide_step_chain_kernel<QD, false>)) return rc;
        hipLaunchKernelGGL((guide_step_chain_kernel<QD, false>), dim3(B), dim3(512), lds, st, ca);
    }
    return 0;
}

int launch_chain_guide(const GuideArgs& a, const float* table, const ChainInfo& ci, bool multi, size_t lds, int B, hipStream_t st) {
    ChainGuideArgs ca;
    ca.g = a; ca.table = table; ca.n_table_floats = ci.n_floats;
    switch (ci.n_joints) {
        case 1: return chain_guide_qd<1>(ca, multi, lds, B, st);
        case 2: return chain_guide_qd<2>(ca, multi, lds, B, st);
        case 3: return chain_guide_qd<3>(ca, multi, lds, B, st);
        case 4: return chain_guide_qd<4>(ca, multi, lds, B, st);
        case 5: return chain_guide_qd<5>(ca, multi, lds, B, st);
        case 6: return chain_guide_qd<6>(ca, multi, lds, B, st);
        case 7: return chain_guide_qd<7>(ca, multi, lds, B, st);
        case 8: return chain_guide_qd<8>(ca, multi, lds, B, st);
    }
    return fail(MPDX_E_INVALID, "chain: n_joints %d", ci.n_joints);
}

template <int QD>
static int chain_metrics_qd(const dev_guide_params& g, const float* x, float* out4, uint8_t* mask, int n_check, int B, int H, const dev_scenes& sc, const float* table,
                            int ntab, bool multi, size_t lds, hipStream_t st) {
    if (multi) {
        if (int rc = raise_lds_limit((const void*)traj_metrics_chain_kernel<QD, true>)) return rc;
        hipLaunchKernelGGL((traj_metrics_chain_kernel<QD, true>), dim3(B), dim3(64), lds, st, g, x, out4, B, H, n_check, mask, sc, table, ntab);
    } else {
        if (int rc = raise_lds_limit((const void*)traj_metrics_chain_kernel<QD, false>)) return rc;
        hipLaunchKernelGGL((traj_metrics_chain_kernel<QD, false>), dim3(B), dim3(64), lds, st, g, x, out4, B, H, n_check, mask, sc, table, ntab);
    }
    return 0;
}

int launch_chain_metrics(const dev_guide_params& g, const float* x, float* out4, uint8_t* mask, int n_check, int B, int H, const dev_scenes& sc, const float* table,
                         const ChainInfo& ci, bool multi, hipStream_t st) {
    const int D = 2 * ci.n_joints;
    const size_t lds = (size_t)(H * D + ((ci.n_floats + 3) & ~3) + 64 * kChainPS + g.n_prim_floats) * sizeof(float);
    if (lds > 160 * 1024) return fail(MPDX_E_INVALID, "chain metrics need %zu B of LDS", lds);
#define MPDX_CM(QD_) case QD_: return chain_metrics_qd<QD_>(g, x, out4, mask, n_check, B, H, sc, table, ci.n_floats, multi, lds, st);
    switch (ci.n_joints) { MPDX_CM(1) MPDX_CM(2) MPDX_CM(3) MPDX_CM(4) MPDX_CM(5) MPDX_CM(6) MPDX_CM(7) MPDX_CM(8) }
#undef MPDX_CM
    return fail(MPDX_E_INVALID, "chain: n_joints %d", ci.n_joints);
}

}  // namespace mpdx
