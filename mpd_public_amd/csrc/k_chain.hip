// k_chain.hip - the guide and trajectory-metrics kernels of a table-driven serial chain (chain.hpp): every instantiation (1 ... 8 joints, one scene
// or several) behind two launchers; k_guide.hip checks the block and dispatches here.
#include "host.hpp"
#include "chain.hpp"

namespace mpdx {

// fn(number of joints, several scenes) as compile-time constants, for n_joints in 1 ... MPDX_ROBOT_CHAIN_MAX_JOINTS (the chain kernels have no grid variant)
template <int QD = 1, class F>
static int with_chain(int n_joints, bool multi, F&& fn) {
    if constexpr (QD > MPDX_ROBOT_CHAIN_MAX_JOINTS) return fail(MPDX_E_INVALID, "chain: n_joints %d", n_joints);
    else return n_joints == QD ? with_bools([&](auto multi_c) { return fn(std::integral_constant<int, QD>{}, multi_c); }, multi) : with_chain<QD + 1>(n_joints, multi, fn);
}

int launch_chain_guide(const GuideArgs& a, const float* table, const ChainInfo& ci, bool multi, size_t lds, int B, hipStream_t st) {
    ChainGuideArgs ca;
    ca.g = a; ca.table = table; ca.n_table_floats = ci.n_floats;
    return with_chain(ci.n_joints, multi, [&](auto qd, auto multi_c) {
        auto kern = guide_step_chain_kernel<decltype(qd)::value, decltype(multi_c)::value>;
        if (int rc = raise_lds_limit((const void*)kern)) return rc;
        hipLaunchKernelGGL(kern, dim3(B), dim3(512), lds, st, ca);
        return 0;
    });
}

int launch_chain_metrics(const dev_guide_params& g, const float* x, float* out4, uint8_t* mask, int n_check, int B, int H, const dev_scenes& sc, const float* table,
                         const ChainInfo& ci, bool multi, hipStream_t st) {
    const size_t lds = metrics_lds_layout(true, H, 2 * ci.n_joints, g.n_prim_floats, ci.n_floats).total * sizeof(float);
    if (lds > 160 * 1024) return fail(MPDX_E_INVALID, "chain metrics need %zu B of LDS", lds);
    return with_chain(ci.n_joints, multi, [&](auto qd, auto multi_c) {
        auto kern = traj_metrics_chain_kernel<decltype(qd)::value, decltype(multi_c)::value>;
        if (int rc = raise_lds_limit((const void*)kern)) return rc;
        hipLaunchKernelGGL(kern, dim3(B), dim3(64), lds, st, g, x, out4, B, H, n_check, mask, sc, table, ci.n_floats);
        return 0;
    });
}

}  // namespace mpdx
