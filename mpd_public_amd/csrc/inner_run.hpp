// inner_run.hpp - runs of consecutive inner-level layers of mpdx_plan as ONE persistent launch each, at small batch.  Two sequences:
//   RunSeqSeven  the seven 256 -> 256 Conv1dBlocks of the innermost level (downs[3].0.blocks[1], downs[3].1, mid_block1, mid_block2);
//   RunSeqTail   the tail of up level 0: the three 128 -> 128 Conv1dBlocks (ups[0].0.blocks[1], ups[0].1.blocks[0], ups[0].1.blocks[1]) and
//                Upsample1d(128), ConvTranspose1d(4, 2, 1) on 8 -> 16 positions, as the run's last layer.
//
// Every GroupNorm layer of a sequence is conv_block_kernel<CONV_S1, 5, EPI_GN_MISH, MT, NT, 1, 8, GeoL8<.>, .> (MT = 32 for 256 channels, 16 for 128),
// the transposed conv conv_block_kernel<CONV_UPT, 4, EPI_BIAS, 16, 2 NT, 1, 8, GeoUp8<8>>: 8 channel tiles x ceil(B / spt) position tiles of spt = NT / 8
// whole trajectories.  NT - the run's WIDTH - is a compile-time parameter of the sequence: 32 (4 trajectories per position tile, one workgroup per CU)
// or 16 (2 trajectories, up to two workgroups per CU: one workgroup's latency phases - poll, sc1 window loads, LDS reduction, one-wave epilogue, store
// drain - under the other's k-loop).  The K split over the 8 waves, the fixed-order reduction and the per-region GroupNorm do not depend on NT, so
// both widths give the per-layer kernels' bits.  A position tile of layer i + 1 needs the 8 workgroups of the SAME position tile of layer i and nothing else of the
// grid, so a workgroup keeps its (channel tile, position tile) for the whole run and the 8 workgroups of a position tile - a cluster - hand their output
// tiles to each other through memory: conv_block_body<.., RUN = true> (conv_block.hpp) stores write-through, counts arrivals in one word per cluster and
// reads handed-off bytes past the L1.  The arithmetic is the per-layer kernels': outputs are equal bit for bit.
//
// Re-used workspace slots.  A workgroup passes the counter of layer i only after all 8 workgroups of its cluster have FINISHED layer i - their reads of
// the layer's input window and residual tile included (the arrival add is the last thing a layer does).  So when it overwrites a slot in layer i + 1,
// no workgroup of the cluster still reads that slot for layer i or before, and the other clusters touch other trajectories: the slot plan that is safe
// across the per-layer launches (where layer i + 1 starts after ALL of layer i) is safe here - as long as every tensor of the run gives a trajectory
// the same bytes of its slot.  Upsample1d's output does not (16 positions: trajectory b lies where trajectories 2 b and 2 b + 1 of an 8-position
// tensor lie), so the host keeps its slot away from every other layer of the run (mpdx.hip tail_run_first: layer 0's output goes to a spare slot).
//
// Every wait is bounded (RunCtx::budget).  A workgroup that gives up sets the handle's sticky status word (system scope, host-mapped), poisons its
// cluster's counter - its peers leave their polls at once and give up too, so the launch ends within one budget - and writes NaN into its tile of the
// run's last output.  The counters are not reset between launches and are shared by the handle's runs: `base` advances by 8 x layers per launch (the
// host zeroes them only when a batch brings more clusters than the launch before, or after a give-up).
#pragma once
#include "conv_block.hpp"

namespace mpdx {

constexpr int kInnerRunLayers = 7;
constexpr int kTailRunLayers = 4;
constexpr int kInnerRunCounterStride = 32;   // words between two clusters' counters: a 128-byte line each
constexpr int kRunWide = 32, kRunNarrow = 16;   // the two widths: positions per cluster (8 per trajectory)

// ---- the launch geometry, stated once for kernel and host.  A cluster is `width / 8` trajectories; cluster c, channel tile m is block
// x + 8 (m + 8 (c / 8)) with x = c % 8: workgroups are dealt round-robin over the 8 XCDs (block b and b + 8 share one), so the 8 workgroups of a
// cluster sit on ONE XCD; the grid is rounded up to whole groups of 8 clusters and the surplus workgroups leave at once.  The cluster-spread
// placement (same_xcd = false: block 8 c + m, channel tile m on XCD m) is kept for A/B builds.  Results do not depend on the placement.
struct RunSlot { int c, m; };
constexpr int run_clusters(int B, int width) { return (B + width / 8 - 1) / (width / 8); }
constexpr int run_grid(int nc, bool same_xcd) { return same_xcd ? ((nc + 7) / 8) * 64 : nc * 8; }
constexpr int run_block(int c, int m, bool same_xcd) { return same_xcd ? (c & 7) + 8 * (m + 8 * (c >> 3)) : 8 * c + m; }
__host__ __device__ constexpr RunSlot run_slot(int block, bool same_xcd) {
    return same_xcd ? RunSlot{((block >> 6) << 3) + (block & 7), (block >> 3) & 7} : RunSlot{block >> 3, block & 7};
}
// every (cluster, channel tile) of a batch of up to 128 is exactly one block of the grid, every other block names a cluster >= nc (it leaves), and the
// 8 blocks of a cluster share block % 8 - their XCD
constexpr bool run_map_ok(int width) {
    for (int B = 1; B <= 128; ++B) {
        const int nc = run_clusters(B, width), grid = run_grid(nc, true);
        int live = 0;
        for (int b = 0; b < grid; ++b) {
            const RunSlot s = run_slot(b, true);
            if (s.m < 0 || s.m > 7 || s.c < 0) return false;
            if (s.c >= nc) continue;
            if (run_block(s.c, s.m, true) != b || (b & 7) != (s.c & 7)) return false;
            ++live;
        }
        if (live != 8 * nc || grid % 64 || grid < 8 * nc) return false;
    }
    return true;
}
static_assert(run_map_ok(kRunWide) && run_map_ok(kRunNarrow), "block <-> (cluster, channel tile): a bijection on the live blocks, one XCD per cluster");

template <int N>
struct RunArgs {
    ConvArgs layer[N];
    unsigned* counters;   // [nc * kInnerRunCounterStride]
    unsigned* status;     // sticky give-up word of the handle: bit 0 set, bits 8.. the layer that waited
    long long budget;     // s_memtime ticks (shader clock) of 4 ms
    unsigned base;        // counter value of every cluster when the launch starts
    int n_layers;
    int nc;               // clusters = position tiles = run_clusters(B, width)
};
typedef RunArgs<kInnerRunLayers> InnerRunArgs;
typedef RunArgs<kTailRunLayers> TailRunArgs;

constexpr size_t run_max(size_t a, size_t b) { return a > b ? a : b; }

// A layer sequence: kGn GroupNorm layers of one kind (gn), then - kUp - one transposed conv (up); the tile of the LAST layer's output per workgroup is
// kSpt trajectories x kLastL positions x kLastMT channels of kLastC.  lds(): max over the sequence of conv_block_lds_bytes + the poll's verdict word.
// NT: the run's width (kRunWide / kRunNarrow).
template <int NT>
struct RunSeqSeven {
    typedef InnerRunArgs Args;
    static constexpr int kWidth = NT, kSpt = NT / 8;
    static constexpr int kLayers = kInnerRunLayers;
    static constexpr bool kUp = false;
    static constexpr int kLastL = 8, kLastMT = 32, kLastC = 256;
    static __device__ __forceinline__ bool gn(const ConvArgs& a, int id, const RunCtx& rc) { return conv_block_body<CONV_S1, 5, EPI_GN_MISH, 32, NT, 1, 8, GeoL8<16>, -1, true>(a, id, rc); }
    static __device__ __forceinline__ bool up(const ConvArgs&, int, const RunCtx&) { return true; }
    static __device__ __forceinline__ int tiled(int) { return 0; }   // 32-channel tiles: a position's 128 bytes are a whole line in [B][8][C]
    static size_t lds() { return conv_block_lds_bytes<CONV_S1, 5, 32, NT, 8>(8, 8, 256 + 8) + 16; }
};
template <int NT>
struct RunSeqTail {
    typedef TailRunArgs Args;
    static constexpr int kWidth = NT, kSpt = NT / 8;
    static constexpr int kLayers = kTailRunLayers;
    static constexpr bool kUp = true;
    static constexpr int kLastL = 16, kLastMT = 16, kLastC = 128;
    static __device__ __forceinline__ bool gn(const ConvArgs& a, int id, const RunCtx& rc) { return conv_block_body<CONV_S1, 5, EPI_GN_MISH, 16, NT, 1, 8, GeoL8<8>, -1, true>(a, id, rc); }
    static __device__ __forceinline__ bool up(const ConvArgs& a, int id, const RunCtx& rc) { return conv_block_body<CONV_UPT, 4, EPI_BIAS, 16, 2 * NT, 1, 8, GeoUp8<8>, -1, true>(a, id, rc); }
    // RunCtx::tiled of layer i: the three GroupNorm outputs are handed over tile-major - layer i > 0 reads its input so, layer 2 (ups.0.1.blocks.1) its
    // residual (layer 0's output), the transposed conv its input; what comes from earlier launches and what leaves the run is [B][L][C]
    static __device__ __forceinline__ int tiled(int i) { return i >= 3 ? 1 : ((i > 0 ? 1 : 0) | (i == 2 ? 2 : 0) | 4); }
    static size_t lds() { return run_max(conv_block_lds_bytes<CONV_S1, 5, 16, NT, 8>(8, 8, 128 + 8), conv_block_lds_bytes<CONV_UPT, 4, 16, 2 * NT, 8>(8, 16, 128 + 4)) + 16; }
};

// A workgroup of cluster c, channel tile m gave up at layer i (uniform over the workgroup).
template <class SEQ>
__device__ __forceinline__ void run_give_up(const typename SEQ::Args& ra, const RunCtx& rc, const int c, const int m, const int i) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        __hip_atomic_fetch_or(ra.status, 1u | ((unsigned)i << 8), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        // (a store, not an add: every workgroup of a cluster that gives up does so at the SAME layer - none can be a layer ahead of one that has
        //  not arrived - so the poison is the same word however many of them write it; a late honest arrival adds 1 to it and leaves it poisoned)
        __hip_atomic_store(rc.counter, rc.target + kRunPoison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // this workgroup's tile of the run's output: kSpt trajectories x kLastL positions x kLastMT channels
    const ConvArgs& last = ra.layer[ra.n_layers - 1];
    constexpr int L = SEQ::kLastL, MT = SEQ::kLastMT;
    for (int e = tid; e < SEQ::kSpt * L * MT; e += 512) {
        const int b = c * SEQ::kSpt + (e >> geo_ilog2(L * MT)), l = (e >> geo_ilog2(MT)) & (L - 1), ch = m * MT + (e & (MT - 1));
        if (b < last.B) last.dst[((size_t)b * L + l) * SEQ::kLastC + ch] = __builtin_nanf("");
    }
}

// SAME_XCD: the placement of run_slot (above).
template <class SEQ, bool SAME_XCD>
__global__ __launch_bounds__(512) void inner_run_kernel(const typename SEQ::Args ra) {
    const RunSlot slot = run_slot((int)blockIdx.x, SAME_XCD);
    const int c = slot.c, m = slot.m;
    if constexpr (SAME_XCD) {
        if (c >= ra.nc) return;
    }
    warm_kernarg<sizeof(typename SEQ::Args)>();
    RunCtx rc;
    rc.counter = ra.counters + (size_t)c * kInnerRunCounterStride;
    rc.budget = ra.budget;
    const int n_gn = SEQ::kUp ? ra.n_layers - 1 : ra.n_layers;   // the transposed conv is the run's last layer
#pragma nounroll
    for (int i = 0; i < n_gn; ++i) {
        rc.wait = i > 0;
        rc.target = ra.base + 8u * (unsigned)i;
        rc.tiled = SEQ::tiled(i);
        if (SEQ::gn(ra.layer[i], c * 8 + m, rc)) continue;
        run_give_up<SEQ>(ra, rc, c, m, i);
        return;
    }
    if constexpr (SEQ::kUp) {
        rc.wait = n_gn > 0;
        rc.target = ra.base + 8u * (unsigned)n_gn;
        rc.tiled = SEQ::tiled(n_gn);
        if (!SEQ::up(ra.layer[n_gn], c * 8 + m, rc)) run_give_up<SEQ>(ra, rc, c, m, n_gn);
    }
}

}  // namespace mpdx
