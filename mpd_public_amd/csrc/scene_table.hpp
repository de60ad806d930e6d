// scene_table.hpp - several obstacle scenes in one launch of the guide / metrics kernels: the trajectories (= workgroups) of a batch see different
// primitive tables (include/mpdx.h, the scene members of mpdx_guide_params).
//
// Replaces nothing in the reference: run_inference plans ONE task per call (scripts/inference/inference.py:107-123 builds one PlanningTask, its
// extra objects included); a batch of requests with different obstacles is this package's extension.
//
// The kernels already stage the primitive table into LDS in their prologue, one workgroup per trajectory: a per-scene table is a different SOURCE
// address for that copy and per-scene loop bounds for the primitive scans, nothing in the hot loops.  A workgroup's scene is wave-uniform: the scene
// index, the block address and the counts are scalar values (uniform loads before the kernel's first global store, readfirstlane).
// MULTI_SCENE is a template parameter of the kernels next to HAS_GRID, chosen by the launcher when n_scenes > 1, so that the single-scene
// instantiations compile from exactly the code they had; the descriptor travels behind dev_grids (dev_guide_params keeps its layout).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mpdx.h"
#include "grid_field.hpp"

namespace mpdx {

struct dev_scenes {
    const int32_t* scene_of_ctx;   // device: scene per group of n_per_ctx trajectories
    int32_t n_scenes;              // > 1 in a MULTI_SCENE launch
    int32_t stride;                // floats per scene block
    int32_t n_per_ctx;             // > 0
    int32_t tail;                  // floats of the shared tail behind the last block (staged behind the workgroup's block)
};

// per-scene primitive counts of the workgroup's scene, clamped to the fields' capacities (scalar registers)
struct SceneCounts {
    int ns[MPDX_MAX_FIELDS], nb[MPDX_MAX_FIELDS];
};

// scene of trajectory b, clamped into [0, n_scenes): a bad table entry selects another scene, never memory outside prims
__device__ __forceinline__ int scene_of_traj(const dev_scenes& sc, int b) {
    const int s = sc.scene_of_ctx[b / sc.n_per_ctx];
    return __builtin_amdgcn_readfirstlane(min(max(s, 0), sc.n_scenes - 1));
}

// the header of scene block `blk` (MPDX_SCENE_HEADER_WORDS int32), each count clamped into [0, capacity of the field]: a scan never leaves the table
__device__ __forceinline__ SceneCounts scene_counts(const dev_guide_params& gp, const float* __restrict__ blk) {
    SceneCounts c;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(blk);
#pragma unroll
    for (int f = 0; f < MPDX_MAX_FIELDS; ++f) {
        c.ns[f] = __builtin_amdgcn_readfirstlane(min(max(hdr[f], 0), gp.fields[f].n_spheres));
        c.nb[f] = __builtin_amdgcn_readfirstlane(min(max(hdr[MPDX_MAX_FIELDS + f], 0), gp.fields[f].n_boxes));
    }
    return c;
}

// field f as the workgroup's scene sees it: the same offsets, the scene's own counts
__device__ __forceinline__ dev_field scene_field(const dev_guide_params& gp, const SceneCounts& c, int f) {
    dev_field fl = gp.fields[f];
    int ns = c.ns[0], nb = c.nb[0];
#pragma unroll
    for (int k = 1; k < MPDX_MAX_FIELDS; ++k) { ns = f == k ? c.ns[k] : ns; nb = f == k ? c.nb[k] : nb; }
    fl.n_spheres = ns; fl.n_boxes = nb;
    return fl;
}

// the LDS image of the workgroup's scene: [block `scene` | shared tail], gp.n_prim_floats = stride + tail floats (set by the launcher)
__device__ __forceinline__ void stage_scene_table(const dev_guide_params& gp, const dev_scenes& sc, int scene, float* __restrict__ sprim, int tid, int nthr) {
    const float* __restrict__ blk = gp.prims + (size_t)scene * sc.stride;
    const float* __restrict__ shared = gp.prims + (size_t)sc.n_scenes * sc.stride;
    for (int i = tid; i < gp.n_prim_floats; i += nthr) sprim[i] = i < sc.stride ? blk[i] : shared[i - sc.stride];
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline bool has_scenes(const mpdx_guide_params& gp) { return gp.n_scenes > 1; }

// floats a workgroup stages: the whole table, or one scene block + the shared tail
inline int staged_prim_floats(const mpdx_guide_params& gp) {
    return has_scenes(gp) ? gp.scene_stride + (gp.n_prim_floats - gp.n_scenes * gp.scene_stride) : gp.n_prim_floats;
}

// The descriptor checks of every launcher that takes scenes: nullptr = fine (or a single scene), else what is wrong.  After them every address the
// staging loop forms lies inside [prims, prims + n_prim_floats) and every table offset inside the staged image.
inline const char* scene_params_problem(const mpdx_guide_params& gp) {
    if (!has_scenes(gp)) return nullptr;
    if (!gp.scene_of_ctx) return "n_scenes > 1 without a scene table (scene_of_ctx == NULL)";
    if (gp.scene_n_per_ctx <= 0) return "scene_n_per_ctx must be positive (trajectories per entry of the scene table)";
    if (!gp.prims) return "n_scenes > 1 without scene blocks (prims == NULL)";
    if (gp.scene_stride <= 0 || (gp.scene_stride & 3)) return "scene_stride must be a positive multiple of 4 floats";
    if (gp.scene_stride < MPDX_SCENE_HEADER_WORDS) return "scene_stride smaller than the scene header";
    if ((long long)gp.n_scenes * gp.scene_stride > (long long)gp.n_prim_floats) return "n_scenes * scene_stride exceeds n_prim_floats (scene blocks beyond the primitive table)";
    const long long staged = (long long)gp.scene_stride + ((long long)gp.n_prim_floats - (long long)gp.n_scenes * gp.scene_stride);
    if (staged > MPDX_SCENE_MAX_STAGED_FLOATS) return "scene block + shared tail exceed the LDS table budget (MPDX_SCENE_MAX_STAGED_FLOATS)";
    for (int i = 0; i < gp.n_fields && i < MPDX_MAX_FIELDS; ++i) {
        const mpdx_field& f = gp.fields[i];
        if (f.kind != MPDX_FIELD_OBJECTS) continue;
        if (f.n_spheres < 0 || f.n_boxes < 0 || f.sphere_off < 0 || f.box_off < 0) return "scene field: negative table offset or capacity";
        const long long tabs[2][2] = {{f.sphere_off, 4ll * f.n_spheres}, {f.box_off, 6ll * f.n_boxes}};
        for (const auto& t : tabs) {
            if (t[1] == 0) continue;
            if (t[0] < gp.scene_stride) {   // a per-scene table: behind the header, inside the block
                if (t[0] < MPDX_SCENE_HEADER_WORDS) return "scene field: a table overlaps the scene header";
                if (t[0] + t[1] > gp.scene_stride) return "scene_stride smaller than the scene header plus the per-scene tables";
            } else if (t[0] + t[1] > staged) return "scene field: a shared table beyond the primitive table";
        }
    }
    return nullptr;
}

// the kernels' descriptor of a VALIDATED block
inline dev_scenes dev_scenes_of(const mpdx_guide_params& gp) {
    dev_scenes d;
    memset(&d, 0, sizeof(d));
    if (!has_scenes(gp)) return d;
    d.scene_of_ctx = gp.scene_of_ctx; d.n_scenes = gp.n_scenes; d.stride = gp.scene_stride; d.n_per_ctx = gp.scene_n_per_ctx;
    d.tail = gp.n_prim_floats - gp.n_scenes * gp.scene_stride;
    return d;
}

// the kernels' parameter block of a launch that may carry scenes: n_prim_floats = what a workgroup stages
inline dev_guide_params dev_params_staged(const mpdx_guide_params& gp) {
    dev_guide_params d = dev_params_of(gp);
    d.n_prim_floats = staged_prim_floats(gp);
    return d;
}

}  // namespace mpdx
