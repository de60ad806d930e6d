// k_edt.hip - the Euclidean distance transform and voxelisation kernels (edt.hpp) and their C-ABI entry points.
#include "host.hpp"
#include "edt.hpp"

namespace mpdx {

static bool edt_finite(float v) { return fabsf(v) < 3.0e38f; }   // (false for NaN)

// the shape checks the three entry points share: 0 and `nodes`, or the failure.  2-D = n[2] == 1.
static int edt_shape(const char* who, const int n[3], long long* nodes) {
    if (!n) return fail(MPDX_E_INVALID, "%s: n is null", who);
    long long t = 1;
    for (int j = 0; j < 3; ++j) {
        const bool ok = j < 2 ? (n[j] >= 2 && n[j] <= 4096) : (n[j] == 1 || (n[j] >= 2 && n[j] <= 4096));
        if (!ok) return fail(MPDX_E_INVALID, "%s: n[%d] = %d (2 ... 4096 along a used axis; n[2] = 1 in 2-D)", who, j, n[j]);
        t *= n[j];
    }
    if (t > (1ll << 29)) return fail(MPDX_E_INVALID, "%s: n gives %lld nodes (at most 2^29)", who, t);
    *nodes = t;
    return 0;
}

// the gradient plane of a finished 3-D sdf plane, for the other producer of grid planes (k_mesh.hip): edt_grad_kernel is instantiated in this TU only
void launch_grid_gradient3(const float* sdf, float* grad, const int n[3], float cell, hipStream_t st) {
    EdtArgs a;
    memset(&a, 0, sizeof(a));
    a.sdf = const_cast<float*>(sdf); a.grad = grad;
    for (int j = 0; j < 3; ++j) a.n[j] = n[j];
    a.nodes = n[0] * n[1] * n[2];
    a.k1 = 1.0f / cell; a.k2 = 0.5f / cell;
    hipLaunchKernelGGL(edt_grad_kernel<3>, dim3((unsigned)((a.nodes + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace mpdx

extern "C" {

size_t mpdx_sdf_grid_edt_ws_bytes(const int n[3]) {
    using namespace mpdx;
    long long nodes;
    if (edt_shape("edt workspace", n, &nodes)) return 0;
    return (size_t)nodes * 2 * sizeof(int32_t);
}

int mpdx_sdf_grid_from_occupancy(const uint8_t* occ, float* sdf_out, float* grad_out, int32_t* d2_out, const int n[3], float cell, float inflate, void* ws,
                                 size_t ws_bytes, void* stream) {
    using namespace mpdx;
    const char* who = "sdf from occupancy";
    if (!occ) return fail(MPDX_E_INVALID, "%s: occ is null", who);
    if (!sdf_out) return fail(MPDX_E_INVALID, "%s: sdf_out is null", who);
    if (!ws) return fail(MPDX_E_INVALID, "%s: ws is null", who);
    long long nodes;
    if (int rc = edt_shape(who, n, &nodes)) return rc;
    if (!(cell > 0.f) || !edt_finite(cell)) return fail(MPDX_E_INVALID, "%s: cell must be positive and finite", who);
    if (!(inflate >= 0.f) || !edt_finite(inflate)) return fail(MPDX_E_INVALID, "%s: inflate must be non-negative and finite", who);
    if (grad_out && ((uintptr_t)grad_out & 15)) return fail(MPDX_E_INVALID, "%s: grad_out must be 16-byte aligned", who);
    if (((uintptr_t)sdf_out & 3) || ((uintptr_t)ws & 3) || ((uintptr_t)d2_out & 3)) return fail(MPDX_E_INVALID, "%s: sdf_out, d2_out and ws must be 4-byte aligned", who);
    if (ws_bytes < (size_t)nodes * 2 * sizeof(int32_t))
        return fail(MPDX_E_INVALID, "%s: ws_bytes %zu below mpdx_sdf_grid_edt_ws_bytes = %zu", who, ws_bytes, (size_t)nodes * 2 * sizeof(int32_t));
    const hipStream_t st = (hipStream_t)stream;
    EdtArgs a;
    memset(&a, 0, sizeof(a));
    a.occ = occ; a.ws = (int32_t*)ws; a.sdf = sdf_out; a.grad = grad_out; a.d2 = d2_out;
    for (int j = 0; j < 3; ++j) a.n[j] = n[j];
    a.nodes = (int)nodes;
    a.none = (n[0] + n[1] + n[2]) * (n[0] + n[1] + n[2]);
    a.cell = cell; a.inflate = inflate; a.k1 = 1.0f / cell; a.k2 = 0.5f / cell;
    const int rows = n[1] * n[2];
    hipLaunchKernelGGL(edt_pass_x_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, a);
    for (int axis = 1; axis < (n[2] > 1 ? 3 : 2); ++axis) {
        EdtLineArgs l;
        memset(&l, 0, sizeof(l));
        l.ws = a.ws; l.nodes = a.nodes; l.nx = n[0]; l.L = n[axis]; l.none = a.none;
        l.line_stride = axis == 1 ? n[0] : n[0] * n[1];
        l.outer_stride = axis == 1 ? n[0] * n[1] : n[0];
        l.xs = 6;
        while ((l.L << l.xs) > EDT_TILE_INTS) --l.xs;                       // 4096 << 1 = 8192 ints: xs >= 1
        while (l.xs > 0 && (1 << (l.xs - 1)) >= n[0]) --l.xs;               // no wider than the row
        const int outer = axis == 1 ? n[2] : n[1];
        auto chunks_at = [&](int xs) { return (n[0] + (1 << xs) - 1) >> xs; };
        while (l.xs > 2 && (long long)chunks_at(l.xs) * outer * 2 < 1024) --l.xs;   // a small grid: narrower tiles, more workgroups
        const int chunks = chunks_at(l.xs);
        hipLaunchKernelGGL(edt_pass_line_kernel, dim3(chunks, outer, 2), dim3(256), (size_t)(l.L << l.xs) * sizeof(int32_t), st, l);
    }
    const unsigned blocks = (unsigned)((nodes + 255) / 256);
    hipLaunchKernelGGL(edt_sdf_kernel, dim3(blocks), dim3(256), 0, st, a);
    if (grad_out) {
        if (n[2] > 1) hipLaunchKernelGGL(edt_grad_kernel<3>, dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(edt_grad_kernel<2>, dim3(blocks), dim3(256), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_occupancy_from_points(const float* points, int n_points, uint8_t* occ, const int n[3], const float origin[3], float cell, void* stream) {
    using namespace mpdx;
    const char* who = "occupancy from points";
    if (n_points < 0) return fail(MPDX_E_INVALID, "%s: n_points %d", who, n_points);
    if (!occ) return fail(MPDX_E_INVALID, "%s: occ is null", who);
    if (!origin) return fail(MPDX_E_INVALID, "%s: origin is null", who);
    long long nodes;
    if (int rc = edt_shape(who, n, &nodes)) return rc;
    if (!(cell > 0.f) || !edt_finite(cell)) return fail(MPDX_E_INVALID, "%s: cell must be positive and finite", who);
    const int dim = n[2] > 1 ? 3 : 2;
    for (int j = 0; j < dim; ++j)
        if (!edt_finite(origin[j])) return fail(MPDX_E_INVALID, "%s: origin must be finite", who);
    if (n_points == 0) return 0;
    if (!points) return fail(MPDX_E_INVALID, "%s: points is null", who);
    if ((uintptr_t)points & 3) return fail(MPDX_E_INVALID, "%s: points must be 4-byte aligned", who);
    VoxelArgs v;
    memset(&v, 0, sizeof(v));
    v.points = points; v.occ = occ; v.n_points = n_points; v.dim = dim; v.inv_cell = 1.0f / cell;
    for (int j = 0; j < 3; ++j) { v.n[j] = n[j]; v.origin[j] = j < dim ? origin[j] : 0.f; }
    hipLaunchKernelGGL(occupancy_from_points_kernel, dim3((n_points + 255) / 256), dim3(256), 0, (hipStream_t)stream, v);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
