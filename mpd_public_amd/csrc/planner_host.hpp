// planner_host.hpp - C-ABI entry points of the baseline planners (csrc/planner.hpp); included by k_planner.hip.
#pragma once
#include "planner.hpp"

namespace mpdx {
// the argument checks launch_guide applies to a guide parameter block, for the planners that copy it into their kernel arguments
// (gn_point / config_hit index gp.fields; the GPMP2 kernel's support-window arithmetic assumes n_interp >= H).  H == 0: no horizon (RRT).
static int check_planner_params(const mpdx_guide_params* gp, int H, int D) {
    if (int rc = guide_block_problem(gp, D, nullptr, H)) return rc;
    if (gp->n_scenes > 1) return fail(MPDX_E_INVALID, "the baseline planners take one scene (n_scenes = %d): scene batches are for the guide and metrics kernels", gp->n_scenes);
    for (int f = 0; f < gp->n_fields; ++f)   // gn_point / config_hit scan primitive tables: a grid field would be skipped silently
        if (gp->fields[f].kind == MPDX_FIELD_GRID) return fail(MPDX_E_INVALID, "grid fields: guide and metrics only (field %d is a MPDX_FIELD_GRID)", f);
    if (H > 0 && gp->interpolate && (gp->n_interp < 2 || gp->n_interp < H || gp->n_interp > 8 * H))
        return fail(MPDX_E_INVALID, "n_interp %d unsupported for H=%d", gp->n_interp, H);
    return 0;
}

// a planner kernel's launch: the LDS limit is raised above 64 KB only
template <class K, class A>
static int launch_planner(K kern, int blocks, int threads, size_t lds, hipStream_t st, const A& a) {
    if (lds > 64 * 1024)
        if (int rc = raise_lds_limit((const void*)kern)) return rc;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), lds, st, a);
    return 0;
}
}  // namespace mpdx

extern "C" {

int mpdx_gpmp_step(const mpdx_guide_params* gp, const mpdx_gpmp_opts* o, float* x, float* delta, float* state, int B, int H, int D, int solve,
                   void* stream) {
    using namespace mpdx;
    if (!gp || !o || !x || !delta || !state || B <= 0) return fail(MPDX_E_INVALID, "null argument");
    if (H < 4 || D != 2 * gp->q_dim) return fail(MPDX_E_INVALID, "GPMP2 step: H=%d D=%d q_dim=%d", H, D, gp->q_dim);
    if (!gp->use_gp || !(gp->dt > 0.f) || !(o->sigma_obs > 0.f))
        return fail(MPDX_E_INVALID, "GPMP2 step needs the GP prior (dt, sigma_gp) and sigma_obs > 0");
    if (int rc = check_planner_params(gp, H, D)) return rc;
    GpmpArgs a;
    memset(&a, 0, sizeof(a));
    a.gp = dev_params_of(*gp); a.x = x; a.delta = delta; a.state = state; a.B = B; a.H = H;
    a.sigma_obs = o->sigma_obs; a.lam_up = o->lambda_up; a.lam_down = o->lambda_down; a.lam_min = o->lambda_min; a.lam_max = o->lambda_max;
    a.step = o->step; a.adaptive = o->adaptive; a.solve = solve;
    const int N = gp->interpolate ? gp->n_interp : H;
    hipStream_t st = (hipStream_t)stream;
    int rc = 0;
    const bool known = with_builtin_robot(*gp, [&](auto qd, auto dim, auto robot) {
        const size_t lds = gpmp_lds_bytes<decltype(qd)::value>(H, N, gp->n_prim_floats);
        if (lds > 160 * 1024) rc = fail(MPDX_E_INVALID, "GPMP2 step needs %zu B of LDS (H=%d, %d points)", lds, H, N);
        else rc = launch_planner(gpmp_lm_kernel<decltype(qd)::value, decltype(dim)::value, decltype(robot)::value>, B, kGpmpThreads, lds, st, a);
    }, false);
    if (!known) return fail(MPDX_E_INVALID, "GPMP2 step: unsupported robot %d / q_dim %d", gp->robot, gp->q_dim);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_rrt_connect(const mpdx_guide_params* gp, const mpdx_rrt_opts* o, const float* start, const float* goal, float* nodes, int32_t* parent,
                     int32_t* count, int32_t* link, int32_t* iters, int n, void* stream) {
    using namespace mpdx;
    if (!gp || !o || !start || !goal || !nodes || !parent || !count || !link || !iters || n <= 0) return fail(MPDX_E_INVALID, "null argument");
    if (o->max_nodes < 2 || o->n_edge_checks < 2 || o->n_edge_checks > kRrtThreads || !(o->step > 0.f))
        return fail(MPDX_E_INVALID, "RRT-Connect: max_nodes %d, n_edge_checks %d, step %g", o->max_nodes, o->n_edge_checks, (double)o->step);
    if (o->max_iters < 0 || o->max_connect_steps < 0)
        return fail(MPDX_E_INVALID, "RRT-Connect: max_iters %d, max_connect_steps %d", o->max_iters, o->max_connect_steps);
    if (int rc = check_planner_params(gp, 0, 2 * gp->q_dim)) return rc;
    RrtArgs a;
    memset(&a, 0, sizeof(a));
    a.gp = dev_params_of(*gp); a.start = start; a.goal = goal; a.nodes = nodes; a.parent = parent; a.count = count; a.link = link; a.iters = iters;
    for (int j = 0; j < 8; ++j) { a.q_lo[j] = o->q_lo[j]; a.q_hi[j] = o->q_hi[j]; }
    a.step = o->step; a.max_nodes = o->max_nodes; a.max_iters = o->max_iters; a.max_connect = o->max_connect_steps; a.n_checks = o->n_edge_checks;
    a.seed = o->seed;
    hipStream_t st = (hipStream_t)stream;
    int rc = 0;
    const bool known = with_builtin_robot(*gp, [&](auto qd, auto dim, auto robot) {
        constexpr int QD = decltype(qd)::value;
        const size_t lds = rrt_lds_bytes<QD>(o->max_nodes, gp->n_prim_floats);
        if (lds > 160 * 1024) rc = fail(MPDX_E_INVALID, "RRT-Connect: %d nodes x %d dims need %zu B of LDS", o->max_nodes, QD, lds);
        else rc = launch_planner(rrt_connect_kernel<QD, decltype(dim)::value, decltype(robot)::value>, n, kRrtThreads, lds, st, a);
    }, false);
    if (!known) return fail(MPDX_E_INVALID, "RRT-Connect: unsupported robot %d / q_dim %d", gp->robot, gp->q_dim);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_rrt_paths(const mpdx_guide_params* gp, const float* start, const float* goal, const float* nodes, const int32_t* parent, const int32_t* link,
                   float* trajs_out, int32_t* path_len, int n, int max_nodes, int H, float dt, int n_edge_checks, int rounds, void* stream) {
    using namespace mpdx;
    if (!gp || !start || !goal || !nodes || !parent || !link || !trajs_out) return fail(MPDX_E_INVALID, "RRT paths: null argument");
    if (n <= 0) return fail(MPDX_E_INVALID, "RRT paths: n %d", n);
    if (max_nodes < 2 || H < 2 || H > 1024 || !(dt > 0.f) || n_edge_checks < 2 || n_edge_checks > kRrtThreads || rounds < 0)
        return fail(MPDX_E_INVALID, "RRT paths: max_nodes %d, H %d, dt %g, n_edge_checks %d, rounds %d", max_nodes, H, (double)dt, n_edge_checks, rounds);
    if (int rc = check_planner_params(gp, 0, 2 * gp->q_dim)) return rc;
    RrtPathArgs a;
    memset(&a, 0, sizeof(a));
    a.gp = dev_params_of(*gp); a.start = start; a.goal = goal; a.nodes = nodes; a.parent = parent; a.link = link; a.out = trajs_out; a.path_len = path_len;
    a.max_nodes = max_nodes; a.H = H; a.n_checks = n_edge_checks; a.rounds = rounds; a.dt = dt;
    hipStream_t st = (hipStream_t)stream;
    int rc = 0;
    const bool known = with_builtin_robot(*gp, [&](auto qd, auto dim, auto robot) {
        constexpr int QD = decltype(qd)::value;
        const size_t lds = rrt_path_lds_bytes<QD>(max_nodes, H, gp->n_prim_floats);
        if (lds > 160 * 1024) rc = fail(MPDX_E_INVALID, "RRT paths: %d nodes x %d dims need %zu B of LDS", max_nodes, QD, lds);
        else rc = launch_planner(rrt_path_kernel<QD, decltype(dim)::value, decltype(robot)::value>, n, kRrtThreads, lds, st, a);
    }, false);
    if (!known) return fail(MPDX_E_INVALID, "RRT paths: unsupported robot %d / q_dim %d", gp->robot, gp->q_dim);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
