// k_chain.hip - the guide and trajectory-metrics kernels of a table-driven serial chain (chain.hpp): every instantiation (1 ... 8 joints, one scene
// or several) behind two launchers; k_guide.hip checks the block and dispatches here.
#include "host.hpp"
#include "chain.hpp"

namespace mpdx {

// fn(number of joints, the booleans given ...) as compile-time constants, for n_joints in 1 ... MPDX_ROBOT_CHAIN_MAX_JOINTS (the chain kernels have no grid variant)
template <int QD = 1, class F, class... Bs>
static int with_chain(int n_joints, F&& fn, Bs... bs) {
    if constexpr (QD > MPDX_ROBOT_CHAIN_MAX_JOINTS) return fail(MPDX_E_INVALID, "chain: n_joints %d", n_joints);
    else return n_joints == QD ? with_bools([&](auto... c) { return fn(std::integral_constant<int, QD>{}, c...); }, bs...) : with_chain<QD + 1>(n_joints, fn, bs...);
}

int launch_chain_guide(const GuideArgs& a, const dev_tool& tool, const float* table, const ChainInfo& ci, bool multi, size_t lds, int B, hipStream_t st) {
    ChainGuideArgs ca;
    ca.g = a; ca.table = table; ca.n_table_floats = ci.n_floats; ca.tool = tool;
    return with_chain(ci.n_joints, [&](auto qd, auto multi_c, auto tool_c) {   // (several scenes, the tool-axis term on)
        auto kern = guide_step_chain_kernel<decltype(qd)::value, decltype(multi_c)::value, decltype(tool_c)::value>;
        if (int rc = raise_lds_limit((const void*)kern)) return rc;
        hipLaunchKernelGGL(kern, dim3(B), dim3(512), lds, st, ca);
        return 0;
    }, multi, tool.frame != 0);
}

int launch_chain_metrics(const dev_guide_params& g, const float* x, float* out4, uint8_t* mask, int n_check, int B, int H, const dev_scenes& sc, const float* table,
                         const ChainInfo& ci, bool multi, hipStream_t st) {
    const size_t lds = metrics_lds_layout(true, H, 2 * ci.n_joints, g.n_prim_floats, ci.n_floats).total * sizeof(float);
    if (lds > 160 * 1024) return fail(MPDX_E_INVALID, "chain metrics need %zu B of LDS", lds);
    return with_chain(ci.n_joints, [&](auto qd, auto multi_c) {
        auto kern = traj_metrics_chain_kernel<decltype(qd)::value, decltype(multi_c)::value>;
        if (int rc = raise_lds_limit((const void*)kern)) return rc;
        hipLaunchKernelGGL(kern, dim3(B), dim3(64), lds, st, g, x, out4, B, H, n_check, mask, sc, table, ci.n_floats);
        return 0;
    }, multi);
}

// the tool-axis figures: the kernel stages the header and the joint records of the table only (the spheres and pairs are not read)
int launch_chain_tool_metrics(const dev_tool& tool, const float* x, float* out2, uint8_t* mask, int n_check, int B, int H, const float* table, const ChainInfo& ci,
                              hipStream_t st) {
    const int ntab = kChainHdr + ci.n_joints * kChainJF;
    const size_t lds = ((size_t)H * 2 * ci.n_joints + (size_t)ntab) * sizeof(float);
    return with_chain(ci.n_joints, [&](auto qd) {
        hipLaunchKernelGGL(traj_tool_chain_kernel<decltype(qd)::value>, dim3(B), dim3(64), lds, st, tool, x, out2, mask, B, H, n_check, table, ntab);
        return 0;
    });
}

}  // namespace mpdx
