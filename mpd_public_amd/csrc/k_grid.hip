// k_grid.hip - the producers of signed-distance grid planes and their C-ABI entry points: the bake from primitives (sdf_grid_bake_kernel, grid_field.hpp),
// the Euclidean distance transform and voxelisation (edt.hpp), the mesh distance / winding-number kernel (mesh_sdf.hpp), and the gradient plane by
// differences the last two share (grid_gradient_kernel, grid_field.hpp), and the depth-camera fusion that feeds the transform (tsdf.hpp).
#include "host.hpp"
#include "edt.hpp"
#include "mesh_sdf.hpp"
#include "tsdf.hpp"
#include "scene_table.hpp"   // has_scenes
#include "motion.hpp"        // field_track_len

namespace mpdx {

constexpr long long MESH_MAX_FACES = 1ll << 20;
constexpr long long MESH_MAX_PAIRS = 1ll << 38;          // nodes x faces of one call: a safety cap, not a tuned value (profiles/mesh_sdf_probe.md)
constexpr long long MESH_MAX_LAUNCH_PAIRS = 1ll << 33;   // ... and of one launch: the host splits the node range

// The checks the entry points share: 0, or the failure.
// Node counts: 2 ... 4096 along a used axis, at most 2^29 nodes (-> nodes).  dim 3: a 3-D grid; 2: a 2-D one (n[2] == 1); 0: either.
static int check_shape(const char* who, const int n[3], int dim, long long* nodes) {
    if (!n) return fail(MPDX_E_INVALID, "%s: n is null", who);
    long long t = 1;
    for (int j = 0; j < 3; ++j) {
        const bool unused = j == 2 && (dim == 2 || (dim == 0 && n[2] == 1));
        if (unused ? n[j] != 1 : (n[j] < 2 || n[j] > 4096))
            return fail(MPDX_E_INVALID, "%s: n[%d] = %d (2 ... 4096 along a used axis; %s)", who, j, n[j],
                        dim == 3 ? "3-D only" : dim == 2 ? "n[2] = 1: the grid is 2-D" : "n[2] = 1 in 2-D");
        t *= n[j];
    }
    if (t > (1ll << 29)) return fail(MPDX_E_INVALID, "%s: n gives %lld nodes (at most 2^29)", who, t);
    *nodes = t;
    return 0;
}

static int check_cell(const char* who, float cell) {
    return cell > 0.f && finite_f(cell) ? 0 : fail(MPDX_E_INVALID, "%s: cell must be positive and finite", who);
}

static int check_inflate(const char* who, float inflate) {
    return inflate >= 0.f && finite_f(inflate) ? 0 : fail(MPDX_E_INVALID, "%s: inflate must be non-negative and finite", who);
}

static int check_origin(const char* who, const float origin[3], int dim) {
    for (int j = 0; j < dim; ++j)
        if (!finite_f(origin[j])) return fail(MPDX_E_INVALID, "%s: origin must be finite", who);
    return 0;
}

static int check_aligned(const char* who, const char* name, const void* p, int bytes) {   // (a null pointer is aligned)
    return ((uintptr_t)p & (uintptr_t)(bytes - 1)) ? fail(MPDX_E_INVALID, "%s: %s must be %d-byte aligned", who, name, bytes) : 0;
}

// the gradient plane of the sdf plane the launches before it on `st` finish
static void launch_grid_gradient(const float* sdf, float* grad, const int n[3], long long nodes, float cell, hipStream_t st) {
    GridGradientArgs g;
    memset(&g, 0, sizeof(g));
    g.sdf = sdf; g.grad = grad; g.nodes = (int)nodes; g.k1 = 1.0f / cell; g.k2 = 0.5f / cell;
    for (int j = 0; j < 3; ++j) g.n[j] = n[j];
    const dim3 blocks((unsigned)((nodes + 255) / 256));
    if (n[2] > 1) hipLaunchKernelGGL(grid_gradient_kernel<3>, blocks, dim3(256), 0, st, g);
    else hipLaunchKernelGGL(grid_gradient_kernel<2>, blocks, dim3(256), 0, st, g);
}

}  // namespace mpdx

extern "C" {

int mpdx_sdf_grid_bake(const mpdx_guide_params* gp, int field, float* sdf_out, float* grad_out, const int n[3], const float origin[3], float cell,
                       void* stream) {
    using namespace mpdx;
    const char* who = "grid bake";
    if (!gp || !sdf_out || !n || !origin) return fail(MPDX_E_INVALID, "null argument");
    if (gp->n_fields < 0 || gp->n_fields > MPDX_MAX_FIELDS || field < 0 || field >= gp->n_fields) return fail(MPDX_E_INVALID, "field %d of %d", field, gp->n_fields);
    const mpdx_field& f = gp->fields[field];
    if (f.kind != MPDX_FIELD_OBJECTS) return fail(MPDX_E_INVALID, "grid bake: field %d is not an OBJECTS field", field);
    if (gp->tool_frame != 0) return fail(MPDX_E_INVALID, "grid bake: tool_frame %d (the tool-axis term belongs to the guide; a grid is baked from an OBJECTS field)", gp->tool_frame);
    for (int k = 0; k < MPDX_MAX_FIELDS; ++k)   // a grid stands for the fixed environment: a moving field cannot be baked
        if (field_track_len(*gp, k) != 0) return fail(MPDX_E_INVALID, "grid bake: fields[%d].track_len = %d (a grid does not move; bake the fixed objects and keep the moving field as primitives)", k, field_track_len(*gp, k));
    if (has_scenes(*gp)) return fail(MPDX_E_INVALID, "grid bake: one scene only (n_scenes = %d): a grid stands for the fixed environment", gp->n_scenes);
    if (gp->ws_dim != 2 && gp->ws_dim != 3) return fail(MPDX_E_INVALID, "grid bake: ws_dim %d", gp->ws_dim);
    if (gp->n_prim_floats > 0 && !gp->prims) return fail(MPDX_E_INVALID, "primitive table missing");
    if (f.n_spheres < 0 || f.n_boxes < 0 || f.sphere_off < 0 || f.box_off < 0 || f.sphere_off + 4 * f.n_spheres > gp->n_prim_floats ||
        f.box_off + 6 * f.n_boxes > gp->n_prim_floats || gp->n_prim_floats > 12 * 1024)
        return fail(MPDX_E_INVALID, "grid bake: the field's primitive tables do not lie inside prims (%d floats, at most 12288)", gp->n_prim_floats);
    long long nodes;
    if (int rc = check_shape(who, n, gp->ws_dim, &nodes)) return rc;
    if (int rc = check_cell(who, cell)) return rc;
    if (int rc = check_aligned(who, "grad_out", grad_out, 16)) return rc;
    GridBakeArgs a;
    memset(&a, 0, sizeof(a));
    a.f = dev_field_of(f); a.prims = gp->prims; a.n_prim_floats = gp->n_prim_floats; a.sdf = sdf_out; a.grad = grad_out; a.cell = cell;
    for (int j = 0; j < 3; ++j) { a.n[j] = n[j]; a.origin[j] = j < gp->ws_dim ? origin[j] : 0.f; }
    const unsigned blocks = (unsigned)((nodes + 255) / 256);
    const size_t lds = (size_t)gp->n_prim_floats * sizeof(float);
    if (gp->ws_dim == 2) hipLaunchKernelGGL(sdf_grid_bake_kernel<2>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(sdf_grid_bake_kernel<3>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t mpdx_sdf_grid_edt_ws_bytes(const int n[3]) {
    using namespace mpdx;
    long long nodes;
    if (check_shape("edt workspace", n, 0, &nodes)) return 0;
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
    if (int rc = check_shape(who, n, 0, &nodes)) return rc;
    if (int rc = check_cell(who, cell)) return rc;
    if (int rc = check_inflate(who, inflate)) return rc;
    if (int rc = check_aligned(who, "grad_out", grad_out, 16)) return rc;
    if (int rc = check_aligned(who, "sdf_out", sdf_out, 4)) return rc;
    if (int rc = check_aligned(who, "d2_out", d2_out, 4)) return rc;
    if (int rc = check_aligned(who, "ws", ws, 4)) return rc;
    if (ws_bytes < (size_t)nodes * 2 * sizeof(int32_t))
        return fail(MPDX_E_INVALID, "%s: ws_bytes %zu below mpdx_sdf_grid_edt_ws_bytes = %zu", who, ws_bytes, (size_t)nodes * 2 * sizeof(int32_t));
    const hipStream_t st = (hipStream_t)stream;
    EdtArgs a;
    memset(&a, 0, sizeof(a));
    a.occ = occ; a.ws = (int32_t*)ws; a.sdf = sdf_out; a.d2 = d2_out;
    for (int j = 0; j < 3; ++j) a.n[j] = n[j];
    a.nodes = (int)nodes;
    a.none = (n[0] + n[1] + n[2]) * (n[0] + n[1] + n[2]);
    a.cell = cell; a.inflate = inflate;
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
    hipLaunchKernelGGL(edt_sdf_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, st, a);
    if (grad_out) launch_grid_gradient(sdf_out, grad_out, n, nodes, cell, st);
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
    if (int rc = check_shape(who, n, 0, &nodes)) return rc;
    if (int rc = check_cell(who, cell)) return rc;
    const int dim = n[2] > 1 ? 3 : 2;
    if (int rc = check_origin(who, origin, dim)) return rc;
    if (n_points == 0) return 0;
    if (!points) return fail(MPDX_E_INVALID, "%s: points is null", who);
    if (int rc = check_aligned(who, "points", points, 4)) return rc;
    VoxelArgs v;
    memset(&v, 0, sizeof(v));
    v.points = points; v.occ = occ; v.n_points = n_points; v.dim = dim; v.inv_cell = 1.0f / cell;
    for (int j = 0; j < 3; ++j) { v.n[j] = n[j]; v.origin[j] = j < dim ? origin[j] : 0.f; }
    hipLaunchKernelGGL(occupancy_from_points_kernel, dim3((n_points + 255) / 256), dim3(256), 0, (hipStream_t)stream, v);
    HIP_TRY(hipGetLastError());
    return 0;
}

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
    long long nodes;
    if (int rc = check_shape(who, n, 3, &nodes)) return rc;
    if (int rc = check_cell(who, cell)) return rc;
    if (int rc = check_inflate(who, inflate)) return rc;
    if (int rc = check_origin(who, origin, 3)) return rc;
    if (sign_mode != MPDX_MESH_SIGN_WINDING && sign_mode != MPDX_MESH_SIGN_NONE) return fail(MPDX_E_INVALID, "%s: sign_mode %d is unknown", who, sign_mode);
    if (sign_mode == MPDX_MESH_SIGN_NONE && wind_out)
        return fail(MPDX_E_INVALID, "%s: wind_out with MPDX_MESH_SIGN_NONE (the winding number is not evaluated in that sign_mode)", who);
    if (int rc = check_aligned(who, "vertices", vertices, 4)) return rc;
    if (int rc = check_aligned(who, "faces", faces, 4)) return rc;
    if (int rc = check_aligned(who, "sdf_out", sdf_out, 4)) return rc;
    if (int rc = check_aligned(who, "wind_out", wind_out, 4)) return rc;
    if (int rc = check_aligned(who, "grad_out", grad_out, 16)) return rc;
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
    if (grad_out) launch_grid_gradient(sdf_out, grad_out, n, nodes, cell, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_tsdf_integrate(const mpdx_depth_camera* cams, int n_cams, const float* spheres, int n_spheres, float* tsdf, float* weight, uint8_t* occ,
                        const int n[3], const float origin[3], float cell, float trunc, float max_weight, void* stream) {
    using namespace mpdx;
    const char* who = "tsdf integrate";
    long long nodes;
    if (int rc = check_shape(who, n, 3, &nodes)) return rc;
    if (!cams) return fail(MPDX_E_INVALID, "%s: cams is null", who);
    if (n_cams < 1 || n_cams > MPDX_TSDF_MAX_CAMS) return fail(MPDX_E_INVALID, "%s: n_cams %d (1 ... %d)", who, n_cams, MPDX_TSDF_MAX_CAMS);
    TsdfArgs a;
    memset(&a, 0, sizeof(a));
    for (int c = 0; c < n_cams; ++c) {
        const mpdx_depth_camera& k = cams[c];
        if (!k.depth) return fail(MPDX_E_INVALID, "%s: cams[%d].depth is null", who, c);
        if (int rc = check_aligned(who, "depth", k.depth, 4)) return rc;
        if (k.width < 1 || k.width > 8192 || k.height < 1 || k.height > 8192)
            return fail(MPDX_E_INVALID, "%s: cams[%d] width %d x height %d (1 ... 8192 each)", who, c, k.width, k.height);
        if (!(k.fx > 0.f && finite_f(k.fx)) || !(k.fy > 0.f && finite_f(k.fy)))
            return fail(MPDX_E_INVALID, "%s: cams[%d] fx and fy must be positive and finite", who, c);
        if (!finite_f(k.cx) || !finite_f(k.cy)) return fail(MPDX_E_INVALID, "%s: cams[%d] cx and cy must be finite", who, c);
        for (int i = 0; i < 12; ++i)
            if (!finite_f(k.cam_from_world[i]) || !finite_f(k.world_from_cam[i]))
                return fail(MPDX_E_INVALID, "%s: cams[%d] cam_from_world and world_from_cam must be finite", who, c);
        if (!finite_f(k.min_depth) || !finite_f(k.max_depth) || k.min_depth < 0.f || !(k.max_depth > k.min_depth))
            return fail(MPDX_E_INVALID, "%s: cams[%d] depth bounds min_depth %g, max_depth %g (0 <= min_depth < max_depth, finite)", who, c,
                        (double)k.min_depth, (double)k.max_depth);
        TsdfCam& t = a.cams[c];
        t.depth = k.depth; t.width = k.width; t.height = k.height; t.fx = k.fx; t.fy = k.fy; t.cx = k.cx; t.cy = k.cy;
        t.min_depth = k.min_depth; t.max_depth = k.max_depth;
        for (int i = 0; i < 12; ++i) { t.A[i] = k.cam_from_world[i]; t.B[i] = k.world_from_cam[i]; }
    }
    if (n_spheres < 0 || n_spheres > MPDX_TSDF_MAX_SPHERES) return fail(MPDX_E_INVALID, "%s: n_spheres %d (0 ... %d)", who, n_spheres, MPDX_TSDF_MAX_SPHERES);
    if (n_spheres > 0 && !spheres) return fail(MPDX_E_INVALID, "%s: spheres is null with n_spheres %d", who, n_spheres);
    for (int k = 0; k < n_spheres; ++k) {
        for (int j = 0; j < 4; ++j)
            if (!finite_f(spheres[4 * k + j])) return fail(MPDX_E_INVALID, "%s: spheres[%d] must be finite", who, k);
        if (spheres[4 * k + 3] < 0.f) return fail(MPDX_E_INVALID, "%s: spheres[%d] radius is negative", who, k);
        for (int j = 0; j < 4; ++j) a.spheres[k][j] = spheres[4 * k + j];
    }
    if (int rc = check_cell(who, cell)) return rc;
    if (!origin) return fail(MPDX_E_INVALID, "%s: origin is null", who);
    if (int rc = check_origin(who, origin, 3)) return rc;
    if (!(trunc > 0.f && finite_f(trunc))) return fail(MPDX_E_INVALID, "%s: trunc must be positive and finite", who);
    if (!(max_weight >= 1.f && max_weight <= 16777216.f)) return fail(MPDX_E_INVALID, "%s: max_weight %g (1 ... 2^24)", who, (double)max_weight);
    if (!tsdf) return fail(MPDX_E_INVALID, "%s: tsdf is null", who);
    if (!weight) return fail(MPDX_E_INVALID, "%s: weight is null", who);
    if (!occ) return fail(MPDX_E_INVALID, "%s: occ is null", who);
    if (int rc = check_aligned(who, "tsdf", tsdf, 4)) return rc;
    if (int rc = check_aligned(who, "weight", weight, 4)) return rc;
    a.tsdf = tsdf; a.weight = weight; a.occ = occ;
    for (int j = 0; j < 3; ++j) { a.n[j] = n[j]; a.origin[j] = origin[j]; }
    a.nodes = (int)nodes; a.n_cams = n_cams; a.n_spheres = n_spheres;
    a.cell = cell; a.trunc = trunc; a.max_weight = max_weight;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
