// motion.hpp - moving obstacles: an MPDX_FIELD_OBJECTS field whose primitives translate rigidly along a time-indexed track (include/mpdx.h, the
// track members of mpdx_field).
//
// Replaces nothing in the reference: its collision fields are static (scripts/inference/inference.py:107-123 builds one PlanningTask whose objects do
// not move during the plan); an obstacle that moves while the robot does - a part on a conveyor, a door - is this package's extension.
//
// A trajectory is already a timed object (support h lies at time h * dt), so the field's offset at interpolated point i is the interpolation of the
// track rows of the point's two supports, o_i = l0 * track[i0] + l1 * track[i1], and every link point p of that trajectory point is tested as
// p' = p - o_i.  The force at p' IS the force on the link point (a translation has an identity Jacobian).  The track lies in prims behind the
// primitive tables, so the kernels' prologue stages it into LDS with them: per point and moving field the cost is two LDS reads, DIM multiply-adds
// and DIM subtractions per link point, against a primitive scan of hundreds of instructions.
// MOVING is a template parameter of the kernels next to HAS_GRID and MULTI_SCENE, chosen by the launcher when a field carries a track, so that
// the static instantiations compile from exactly the code they had; the descriptor travels behind dev_grids and dev_scenes (dev_guide_params keeps its
// layout) and only in the arguments of the MOVING instantiations of the guide kernels.  MOVING is instantiated with MULTI_SCENE = false only: the
// host refuses the combination.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/mpdx.h"
#include "guide_common.hpp"

namespace mpdx {

struct dev_motion {
    int32_t off[MPDX_MAX_FIELDS];   // float offset of field f's track in the staged primitive table (a multiple of 4)
    int32_t len[MPDX_MAX_FIELDS];   // 0: field f does not move; else H of the launch
};

// o_i of one track for the point whose interpolation pair is ip: the pair and the arithmetic of q_i = l0 * x[i0] + l1 * x[i1], in fp32.
// VEC4: the staged table is 16-byte aligned (the Panda's carve) - one 16-byte LDS read per row; otherwise DIM dword reads (oz of a 2-D row is not read).
template <int DIM, bool VEC4>
__device__ __forceinline__ void track_offset(const float* __restrict__ sprim, int off, const InterpPair& ip, float (&o)[DIM]) {
    const float* t = sprim + off;
    if constexpr (VEC4) {
        const f32x4 r0 = *(const f32x4*)(t + 4 * ip.i0), r1 = *(const f32x4*)(t + 4 * ip.i1);
#pragma unroll
        for (int j = 0; j < DIM; ++j) o[j] = ip.l0 * r0[j] + ip.l1 * r1[j];
    } else {
        float r0[DIM], r1[DIM];
#pragma unroll
        for (int j = 0; j < DIM; ++j) { r0[j] = t[4 * ip.i0 + j]; r1[j] = t[4 * ip.i1 + j]; }
#pragma unroll
        for (int j = 0; j < DIM; ++j) o[j] = ip.l0 * r0[j] + ip.l1 * r1[j];
    }
}

// len / off of field f from a kernel's optional trailing descriptor (none: the static instantiations, nothing moves)
template <class... M>
__device__ __forceinline__ int track_len_of(int f, const M&... m) {
    if constexpr (sizeof...(M) > 0) return (m.len[f], ...);
    else return 0;
}
template <class... M>
__device__ __forceinline__ int track_off_of(int f, const M&... m) {
    if constexpr (sizeof...(M) > 0) return (m.off[f], ...);
    else return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host side
// The rows of field f's track as the block states them: the track members of mpdx_field share their words with a grid's plane offsets, so a
// MPDX_FIELD_GRID field has none; fields at and beyond n_fields are not looked at.
inline int field_track_len(const mpdx_guide_params& gp, int f) {
    if (f < 0 || f >= gp.n_fields || f >= MPDX_MAX_FIELDS || gp.fields[f].kind == MPDX_FIELD_GRID) return 0;
    return gp.fields[f].track_len;
}
inline bool has_motion(const mpdx_guide_params& gp) {
    for (int f = 0; f < MPDX_MAX_FIELDS; ++f)
        if (field_track_len(gp, f) != 0) return true;
    return false;
}

// The checks of the track members, on members only (nothing is dereferenced): nullptr = fine or no track, else what is wrong, naming the member.
// After them every LDS address the MOVING kernels form from a track lies inside the staged table: rows 0 ... H - 1 of a track that ends inside
// n_prim_floats.  H: the support points of the launch.
inline const char* motion_params_problem(const mpdx_guide_params& gp, int H) {
    static thread_local char msg[200];
    if (!has_motion(gp)) return nullptr;
    for (int f = 0; f < MPDX_MAX_FIELDS; ++f) {
        const int len = field_track_len(gp, f);
        if (len == 0) continue;
        const int off = gp.fields[f].track_off;
        if (gp.n_scenes > 1) { snprintf(msg, sizeof(msg), "fields[%d].track_len = %d with n_scenes = %d: a track needs a single scene", f, len, gp.n_scenes); return msg; }
        if (gp.robot == MPDX_ROBOT_CHAIN) { snprintf(msg, sizeof(msg), "fields[%d].track_len = %d with robot == MPDX_ROBOT_CHAIN: tracks are for the point mass and the Panda", f, len); return msg; }
        if (gp.fields[f].kind != MPDX_FIELD_OBJECTS) { snprintf(msg, sizeof(msg), "fields[%d].track_len = %d: field %d is not an MPDX_FIELD_OBJECTS field", f, len, f); return msg; }
        if (len != H) { snprintf(msg, sizeof(msg), "fields[%d].track_len = %d must be 0 or H of the launch (%d)", f, len, H); return msg; }
        if (off < 0 || (off & 3)) { snprintf(msg, sizeof(msg), "fields[%d].track_off = %d must be a non-negative multiple of 4 floats", f, off); return msg; }
        if (!gp.prims || (long long)off + 4ll * len > (long long)gp.n_prim_floats) {
            snprintf(msg, sizeof(msg), "fields[%d].track_off = %d: the track (%d rows of 4 floats) does not end inside n_prim_floats (%d)", f, off, len, gp.n_prim_floats);
            return msg;
        }
        const long long t0 = off, t1 = (long long)off + 4ll * len;
        for (int k = 0; k < gp.n_fields && k < MPDX_MAX_FIELDS; ++k) {
            const mpdx_field& fl = gp.fields[k];
            if (fl.kind != MPDX_FIELD_OBJECTS) continue;
            const long long tabs[2][2] = {{fl.sphere_off, 4ll * fl.n_spheres}, {fl.box_off, 6ll * fl.n_boxes}};
            for (const auto& t : tabs)
                if (t[1] > 0 && t[0] < t1 && t0 < t[0] + t[1]) { snprintf(msg, sizeof(msg), "fields[%d].track_off = %d: the track overlaps a primitive table of field %d", f, off, k); return msg; }
        }
        for (int k = 0; k < f; ++k) {
            if (field_track_len(gp, k) == 0) continue;
            const long long u0 = gp.fields[k].track_off, u1 = u0 + 4ll * gp.fields[k].track_len;
            if (u0 < t1 && t0 < u1) { snprintf(msg, sizeof(msg), "fields[%d].track_off = %d: the track overlaps the track of field %d", f, off, k); return msg; }
        }
    }
    return nullptr;
}

// fn(MULTI_SCENE, MOVING) as bool constants: one static scene, several scenes, or tracks - never both (motion_params_problem refuses it), so the
// combination is not instantiated
template <class F>
inline auto with_scene_mode(F&& fn, bool multi, bool moving) {
    return moving ? fn(std::false_type{}, std::true_type{}) : multi ? fn(std::true_type{}, std::false_type{}) : fn(std::false_type{}, std::false_type{});
}

// the kernels' descriptor of a VALIDATED block
inline dev_motion dev_motion_of(const mpdx_guide_params& gp) {
    dev_motion d;
    memset(&d, 0, sizeof(d));
    for (int f = 0; f < MPDX_MAX_FIELDS; ++f)
        if (field_track_len(gp, f) != 0) { d.off[f] = gp.fields[f].track_off; d.len[f] = gp.fields[f].track_len; }
    return d;
}

}  // namespace mpdx
