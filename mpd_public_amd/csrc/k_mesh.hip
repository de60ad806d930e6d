// k_mesh.hip - the mesh distance / winding-number kernel (mesh_sdf.hpp) and its C-ABI entry point.
#include "host.hpp"
#include "mesh_sdf.hpp"

namespace mpdx {

static bool mesh_finite(float v) { return fabsf(v) < 3.0e38f; }   // (false for NaN)

constexpr long long MESH_MAX_FACES = 1ll << 20;
constexpr long long MESH_MAX_PAIRS = 1ll << 38;          // nodes x faces of one call: a safety cap, not a tuned value (profiles/mesh_sdf_probe.md)
constexpr long long MESH_MAX_LAUNCH_PAIRS = 1ll << 33;   // ... and of one launch: the host splits the node range

}  // namespace mpdx

extern "C" {

int mpdx_sdf_grid_from_mesh(const float* vertices, int n_vertices, const int32_t* faces, int n_faces, float* sdf_out, float* grad_out, float* wind_out,
                            const int n[3], const float origin[3], float cell, float inflate, int sign_mode, void* stream) {
    using namespace mpdx;
    const char* who = "sdf from mesh";
    if (!vertices) return fail(MPDX_E_INVALID, "%s: vertices is null", who);
    if (!faces) return fail(MPDX_E_INVALID, "%s: faces is null", who);
    if (!sdf_out) return fail(MPDX_E_INVALID, "%s: sdf_out is null", who);
    if (!n) return fail(MPDX_E_INVALID, "%s: n is null", who);
    if (!origin) return fail(MPDX_E_INVALID, "%s: origin is null", who);
    if (n_vertices < 3) return fail(MPDX_E_INVALID, "%s: n_vertices %d (at least 3)", who, n_vertices);
    if (n_faces < 1 || n_faces > MESH_MAX_FACES) return fail(MPDX_E_INVALID, "%s: n_faces %d (1 ... 2^20)", who, n_faces);
    long long nodes = 1;
    for (int j = 0; j < 3; ++j) {
        if (j == 2 && n[2] == 1) return fail(MPDX_E_INVALID, "%s: n[2] = 1: a mesh grid is 3-D only", who);
        if (n[j] < 2 || n[j] > 4096) return fail(MPDX_E_INVALID, "%s: n[%d] = %d (2 ... 4096 along every axis; 3-D only)", who, j, n[j]);
        nodes *= n[j];
    }
    if (nodes > (1ll << 29)) return fail(MPDX_E_INVALID, "%s: n gives %lld nodes (at most 2^29)", who, nodes);
    if (!(cell > 0.f) || !mesh_finite(cell)) return fail(MPDX_E_INVALID, "%s: cell must be positive and finite", who);
    if (!(inflate >= 0.f) || !mesh_finite(inflate)) return fail(MPDX_E_INVALID, "%s: inflate must be non-negative and finite", who);
    for (int j = 0; j < 3; ++j)
        if (!mesh_finite(origin[j])) return fail(MPDX_E_INVALID, "%s: origin must be finite", who);
    if (sign_mode != MPDX_MESH_SIGN_WINDING && sign_mode != MPDX_MESH_SIGN_NONE) return fail(MPDX_E_INVALID, "%s: sign_mode %d is unknown", who, sign_mode);
    if (sign_mode == MPDX_MESH_SIGN_NONE && wind_out)
        return fail(MPDX_E_INVALID, "%s: wind_out with MPDX_MESH_SIGN_NONE (the winding number is not evaluated in that sign_mode)", who);
    if ((uintptr_t)vertices & 3) return fail(MPDX_E_INVALID, "%s: vertices must be 4-byte aligned", who);
    if ((uintptr_t)faces & 3) return fail(MPDX_E_INVALID, "%s: faces must be 4-byte aligned", who);
    if ((uintptr_t)sdf_out & 3) return fail(MPDX_E_INVALID, "%s: sdf_out must be 4-byte aligned", who);
    if ((uintptr_t)wind_out & 3) return fail(MPDX_E_INVALID, "%s: wind_out must be 4-byte aligned", who);
    if ((uintptr_t)grad_out & 15) return fail(MPDX_E_INVALID, "%s: grad_out must be 16-byte aligned", who);
    if (nodes * n_faces > MESH_MAX_PAIRS)
        return fail(MPDX_E_INVALID, "%s: %lld nodes x n_faces %d exceed 2^38 node-face pairs: use a coarser grid or a decimated mesh", who, nodes, n_faces);
    const hipStream_t st = (hipStream_t)stream;
    MeshArgs m;
    memset(&m, 0, sizeof(m));
    m.vertices = vertices; m.faces = faces; m.sdf = sdf_out; m.wind = wind_out; m.n_vertices = n_vertices; m.n_faces = n_faces;
    for (int j = 0; j < 3; ++j) { m.n[j] = n[j]; m.origin[j] = origin[j]; }
    m.cell = cell; m.inflate = inflate;
    // node ranges of whole workgroups, at most 2^33 pairs each (n_faces <= 2^20: at least 8192 nodes)
    const long long per_launch = std::max<long long>(MESH_BLOCK_NODES, MESH_MAX_LAUNCH_PAIRS / n_faces / MESH_BLOCK_NODES * MESH_BLOCK_NODES);
    for (long long begin = 0; begin < nodes; begin += per_launch) {
        m.node_begin = (int)begin;
        m.node_end = (int)std::min(nodes, begin + per_launch);
        const unsigned blocks = (unsigned)((m.node_end - m.node_begin + MESH_BLOCK_NODES - 1) / MESH_BLOCK_NODES);
        if (sign_mode == MPDX_MESH_SIGN_WINDING) hipLaunchKernelGGL(mesh_sdf_kernel<true>, dim3(blocks), dim3(256), 0, st, m);
        else hipLaunchKernelGGL(mesh_sdf_kernel<false>, dim3(blocks), dim3(256), 0, st, m);
    }
    if (grad_out)
        launch_grid_gradient3(sdf_out, grad_out, n, cell, st);   // edt_grad_kernel<3>: the difference formula of the occupancy grids
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
