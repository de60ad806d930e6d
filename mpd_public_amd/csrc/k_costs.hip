// k_costs.hip - the cost-value kernel (costs.hpp): its 11 instantiations (point mass 2-D / 3-D, Panda, chain with 1 ... 8 joints) and the C-ABI
// entry point mpdx_traj_costs.  The block checks are the guide's and the metrics' (guide_block_problem, k_guide.hip).
#include "host.hpp"
#include "costs.hpp"

namespace mpdx {

template <int QD, int DIM, int ROBOT>
static int launch_costs_as(const CostArgs& a, size_t lds, hipStream_t st) {
    auto kern = traj_costs_kernel<QD, DIM, ROBOT>;
    if (lds > 48 * 1024)
        if (int rc = raise_lds_limit((const void*)kern)) return rc;
    hipLaunchKernelGGL(kern, dim3(a.B), dim3(64), lds, st, a);
    return 0;
}

template <int QD = 1>
static int launch_costs_chain(int n_joints, const CostArgs& a, size_t lds, hipStream_t st) {
    if constexpr (QD > MPDX_ROBOT_CHAIN_MAX_JOINTS) return fail(MPDX_E_INVALID, "chain: n_joints %d", n_joints);
    else return n_joints == QD ? launch_costs_as<QD, 3, MPDX_ROBOT_CHAIN>(a, lds, st) : launch_costs_chain<QD + 1>(n_joints, a, lds, st);
}

int launch_traj_costs(const CostArgs& a, const ChainInfo& ci, hipStream_t st) {
    const dev_guide_params& g = a.gp;
    const bool chain = g.robot == MPDX_ROBOT_CHAIN;
    const size_t lds = metrics_lds_layout(g.robot != MPDX_ROBOT_POINTMASS, a.H, 2 * g.q_dim, g.n_prim_floats, chain ? ci.n_floats : 0).total * sizeof(float);
    if (lds > 160 * 1024) return fail(MPDX_E_INVALID, "mpdx_traj_costs needs %zu B of LDS for H = %d and %d table floats (at most 160 KB)", lds, a.H, g.n_prim_floats);
    if (chain) return launch_costs_chain(ci.n_joints, a, lds, st);
    if (g.robot == MPDX_ROBOT_POINTMASS && g.q_dim == 2 && g.ws_dim == 2) return launch_costs_as<2, 2, MPDX_ROBOT_POINTMASS>(a, lds, st);
    if (g.robot == MPDX_ROBOT_POINTMASS && g.q_dim == 3 && g.ws_dim == 3) return launch_costs_as<3, 3, MPDX_ROBOT_POINTMASS>(a, lds, st);
    if (g.robot == MPDX_ROBOT_PANDA && g.q_dim == 7 && g.ws_dim == 3) return launch_costs_as<7, 3, MPDX_ROBOT_PANDA>(a, lds, st);
    return fail(MPDX_E_INVALID, "unsupported robot %d / q_dim %d / ws_dim %d", g.robot, g.q_dim, g.ws_dim);
}

}  // namespace mpdx

using namespace mpdx;

extern "C" {

int mpdx_traj_costs(const mpdx_guide_params* gp, const float* x_unnormalised, float* cost_out, float* clearance_out, float* point_out, int n_points, int B,
                    int H, int D, void* stream) {
    if (!gp) return fail(MPDX_E_INVALID, "mpdx_traj_costs: gp is NULL");
    if (!x_unnormalised) return fail(MPDX_E_INVALID, "mpdx_traj_costs: x_unnormalised is NULL");
    if (!cost_out) return fail(MPDX_E_INVALID, "mpdx_traj_costs: cost_out is NULL");
    if (B <= 0) return fail(MPDX_E_INVALID, "mpdx_traj_costs: B = %d must be positive", B);
    if (D != 2 * gp->q_dim) return fail(MPDX_E_INVALID, "mpdx_traj_costs: D = %d != 2 * q_dim (%d)", D, gp->q_dim);
    if (H < 2) return fail(MPDX_E_INVALID, "mpdx_traj_costs: H = %d: at least 2 support points", H);
    if (n_points != 0 && (n_points < 2 || n_points > 8192)) return fail(MPDX_E_INVALID, "mpdx_traj_costs: n_points = %d outside {0} and 2 ... 8192", n_points);
    ChainInfo chain_info;
    if (int rc = guide_block_problem(gp, D, &chain_info, H)) return rc;   // (the chain table, the grid, scene, track and tool members)
    const int N = n_points ? n_points : gp->interpolate ? gp->n_interp : H;
    if (N < 2 || N > 8192) return fail(MPDX_E_INVALID, "mpdx_traj_costs: n_points = 0 takes n_interp = %d of the block, which is outside 2 ... 8192", N);
    CostArgs a;
    memset(&a, 0, sizeof(a));
    a.gp = dev_params_staged(*gp);
    a.x = x_unnormalised; a.cost = cost_out; a.clearance = clearance_out; a.point = point_out;
    a.B = B; a.H = H; a.N = N;
    if (has_grid_field(*gp)) a.grid = dev_grids_of(*gp);
    a.scene = dev_scenes_of(*gp);
    a.motion = dev_motion_of(*gp);
    a.tool = dev_tool_of(*gp);
    if (gp->robot == MPDX_ROBOT_CHAIN) { a.table = gp->chain; a.ntab = chain_info.n_floats; }
    if (int rc = launch_traj_costs(a, chain_info, (hipStream_t)stream)) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
