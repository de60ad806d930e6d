// inner_run.hpp - the seven consecutive 256 -> 256 Conv1dBlocks of the innermost level (downs[3].0.blocks[1], downs[3].1, mid_block1, mid_block2)
// as ONE persistent launch of mpdx_plan at small batch.
//
// Every one of these layers is conv_block_kernel<CONV_S1, 5, EPI_GN_MISH, 32, 32, 1, 8, GeoL8<16>, .>: 8 channel tiles x ceil(B / 4) position tiles,
// one workgroup per CU.  A position tile of layer i + 1 needs the 8 workgroups of the SAME position tile of layer i and nothing else of the grid, so a
// workgroup keeps its (channel tile, position tile) for the whole run and the 8 workgroups of a position tile - a cluster - hand their output tiles to
// each other through memory: conv_block_body<.., RUN = true> (conv_block.hpp) stores write-through, counts arrivals in one word per cluster and reads
// handed-off bytes past the L1.  The arithmetic is the per-layer kernels': outputs are equal bit for bit.
//
// Re-used workspace slots.  A workgroup passes the counter of layer i only after all 8 workgroups of its cluster have FINISHED layer i - their reads of
// the layer's input window and residual tile included (the arrival add is the last thing a layer does).  So when it overwrites a slot in layer i + 1,
// no workgroup of the cluster still reads that slot for layer i or before, and the other clusters touch other trajectories: the slot plan that is safe
// across the per-layer launches (where layer i + 1 starts after ALL of layer i) is safe here.
//
// Every wait is bounded (RunCtx::budget).  A workgroup that gives up sets the handle's sticky status word (system scope, host-mapped), poisons its
// cluster's counter - its peers leave their polls at once and give up too, so the launch ends within one budget - and writes NaN into its tile of the
// run's last output.  The counters are not reset between launches: `base` advances by 8 x layers per launch (the host zeroes them only when
// a batch brings more clusters than the launch before, or after a give-up).
#pragma once
#include "conv_block.hpp"

namespace mpdx {

constexpr int kInnerRunLayers = 7;
constexpr int kInnerRunCounterStride = 32;   // words between two clusters' counters: a 128-byte line each

struct InnerRunArgs {
    ConvArgs layer[kInnerRunLayers];
    unsigned* counters;   // [nc * kInnerRunCounterStride]
    unsigned* status;     // sticky give-up word of the handle: bit 0 set, bits 8.. the layer that waited
    long long budget;     // s_memtime ticks (shader clock) of 4 ms
    unsigned base;        // counter value of every cluster when the launch starts
    int n_layers;
    int nc;               // clusters = position tiles = ceil(B / 4)
};

// LDS: the staged window of 4 trajectories (12 rows of 256 + 8 floats each; the K-partial buffer is smaller) + the poll's verdict word
constexpr size_t kInnerRunLds = (size_t)4 * 12 * (256 + 8) * sizeof(float) + 16;

// SAME_XCD: workgroups are dealt round-robin over the 8 XCDs (block b and b + 8 share one), so block b = x + 8 * (m + 8 * (c / 8)) with x = c % 8 puts the
// 8 workgroups of cluster c on one XCD (the grid is rounded up to whole groups of 8 clusters; surplus workgroups leave at once).  Otherwise block
// b = 8 c + m: channel tile m on XCD m - a channel tile's weights stay in one L2 - and a cluster spread over all 8.  Results do not depend on it.
template <bool SAME_XCD>
__global__ __launch_bounds__(512) void inner_run_kernel(const InnerRunArgs ra) {
    int c, m;
    if constexpr (SAME_XCD) {
        const int b = blockIdx.x, x = b & 7, r = b >> 3;
        m = r & 7; c = (r >> 3) * 8 + x;
        if (c >= ra.nc) return;
    } else {
        c = (int)blockIdx.x >> 3; m = blockIdx.x & 7;
    }
    warm_kernarg<sizeof(InnerRunArgs)>();
    RunCtx rc;
    rc.counter = ra.counters + (size_t)c * kInnerRunCounterStride;
    rc.budget = ra.budget;
#pragma nounroll
    for (int i = 0; i < ra.n_layers; ++i) {
        rc.wait = i > 0;
        rc.target = ra.base + 8u * (unsigned)i;
        if (conv_block_body<CONV_S1, 5, EPI_GN_MISH, 32, 32, 1, 8, GeoL8<16>, -1, true>(ra.layer[i], c * 8 + m, rc)) continue;
        // gave up (uniform over the workgroup)
        const int tid = threadIdx.x;
        if (tid == 0) {
            __hip_atomic_fetch_or(ra.status, 1u | ((unsigned)i << 8), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            // (a store, not an add: every workgroup of a cluster that gives up does so at the SAME layer - none can be a layer ahead of one that has
            //  not arrived - so the poison is the same word however many of them write it; a late honest arrival adds 1 to it and leaves it poisoned)
            __hip_atomic_store(rc.counter, rc.target + kRunPoison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const ConvArgs& last = ra.layer[ra.n_layers - 1];
        for (int e = tid; e < 4 * 8 * 32; e += 512) {   // this workgroup's tile of the run's output: 4 trajectories x 8 positions x 32 channels
            const int b = c * 4 + (e >> 8), l = (e >> 5) & 7, ch = m * 32 + (e & 31);
            if (b < last.B) last.dst[((size_t)b * 8 + l) * 256 + ch] = __builtin_nanf("");
        }
        return;
    }
}

}  // namespace mpdx
