// switches.hpp - every process-environment switch of libmpdx.so, declared ONCE.  With none of them set the library runs its default
// paths.  Nothing else under csrc/ calls getenv: a call site reads sw::train_gn_fuse() / sw::ksplit(), generated from the table below
// (INTEGRATION.md "Environment switches of libmpdx.so" is the same table for users; tests/test_switches_cpu.py holds the two together).
// Plain C++17 on standard headers, no HIP: it compiles with the host compiler alone.
//
// A row is  X(accessor, "NAME", kind, default, timing, "what it does").
//   kind    PRESENT  bool      set at all, whatever the value (NAME=0 counts as set); default false
//           ON       bool      on unless set to something whose atoi is 0 (NAME=0, NAME= and NAME=x are all OFF); default true
//           INT      int       atoi of the value, the default when unset
//           UINT     unsigned  strtoul of the value with base 0 (0x.. is hexadecimal), the default when unset
//           STR      char*     the value itself, nullptr when unset; the call site parses it
//   timing  ONCE     cached at the first read of THAT switch (a function-local static of its accessor: one copy in the library however
//                    many translation units include this header); set it before the first call of the path it steers
//           LIVE     getenv on every read: tests and A/B runs flip it inside one process
// What a value MEANS beyond its kind (a threshold, an inverted sense, a "%dx%d" tile) stays at the call site or in a helper beside it.
#pragma once
#include <climits>
#include <cstdlib>

namespace mpdx {
namespace sw __attribute__((visibility("hidden"))) {   // (the accessors and their cached values are no symbols of the shared library)

constexpr int kUnset = INT_MIN;   // default of an INT switch that has to tell "not set" from every value a user would write

// clang-format off
#define MPDX_SWITCHES(X) \
    /* ---- diagnostics */ \
    X(debug,               "MPDX_DEBUG",                INT,     0,       ONCE, "1: hipGetLastError() after every launch group of mpdx_plan; 2: also synchronise the stream there, so that an asynchronous fault is attributed to the step that caused it (off: the plan never synchronises)") \
    X(debug_fuse,          "MPDX_DEBUG_FUSE",           STR,     nullptr, LIVE, "set: print every fused segment built and which shape constraint rejected one; a value >= 2 also dumps the segment's LDS geometry as a fused_geom.hpp initialiser") \
    X(debug_train,         "MPDX_DEBUG_TRAIN",          PRESENT, false,   LIVE, "print which backward programs a training pass ran, how many late weight-gradient jobs it collected and the tiles of its input-gradient convolutions (tests/test_gpu_train.py reads the first line, tests/test_gpu_train_batches.py all three)") \
    X(bwd_dbg,             "MPDX_BWD_DBG",              INT,     0,       LIVE, "BwdArgs::dbg of the backward programs (fused_bwd.hpp debug output)") \
    /* ---- path selection (tests and A/B runs use these) */ \
    X(fused,               "MPDX_FUSED",                ON,      true,    LIVE, "0: no fused level program, every layer its own launch (forward of planning and training)") \
    X(fused_mask,          "MPDX_FUSED_MASK",           UINT,    0xffffffffu, LIVE, "bit k enables fused segment k (MPDX_FUSED=0 wins)") \
    X(ws,                  "MPDX_WS",                   INT,     1,       LIVE, "weight-stationary persistent kernels of the inner levels at large batch: 0 off, 2 single layers only (no k5 + 1x1 pairs)") \
    X(wsn,                 "MPDX_WSN",                  ON,      true,    LIVE, "0: the 128-channel layers stay on the per-layer kernels (conv_wsn_kernel off)") \
    X(wsp,                 "MPDX_WSP",                  ON,      true,    LIVE, "0: the 128 -> 256 k5 + 1x1 pair stays on conv_pair_kernel (conv_wsp_kernel off)") \
    X(geo,                 "MPDX_GEO",                  ON,      true,    LIVE, "0: the runtime-geometry kernels instead of the compile-time-geometry ones of the inner levels (conv_block.hpp GeoL8)") \
    X(no_merge,            "MPDX_NO_MERGE",             PRESENT, false,   LIVE, "one fused program per U-Net level: neither the outer down levels nor the outer up levels merge") \
    X(no_merge_up,         "MPDX_NO_MERGE_UP",          PRESENT, false,   LIVE, "the two outer up levels + final_conv + DDPM step stay two programs") \
    X(merge_down3,         "MPDX_MERGE_DOWN3",          ON,      true,    LIVE, "0: four levels keep downs.0 + downs.1 and downs.2 apart (merged, 15 ops: cfg 2 23.10 -> 22.47 ms, cfg 5 shard 624 -> 617 ms)") \
    X(no_mid2,             "MPDX_NO_MID2",              PRESENT, false,   LIVE, "four levels: the third down level (C = 128, L = 16) per layer, not as its own program") \
    X(no_mid3,             "MPDX_NO_MID3",              PRESENT, false,   LIVE, "three levels: the innermost level + the two middle blocks per layer, not as one program (nine launches of ~4.8 us: 43 us of a batch-32 training iteration)") \
    X(static_programs,     "MPDX_STATIC_PROGRAMS",      ON,      true,    ONCE, "0: every fused segment on the generic op-list kernel (runtime descriptors), none as a static program") \
    X(pair,                "MPDX_PAIR",                 ON,      true,    ONCE, "0: blocks[0] and the residual 1x1 convolution of a ResidualTemporalBlock as two launches (conv_pair_kernel off)") \
    X(guide_dense,         "MPDX_GUIDE_DENSE",          INT,     -1,      ONCE, "Panda guide, dense variant (no FK table, 128 VGPRs: two workgroups per CU): 0 / 1 force it off / on, -1 from batch 512 on") \
    /* ---- tile and launch-shape overrides (development) */ \
    X(tile,                "MPDX_TILE",                 STR,     nullptr, ONCE, "MTxNT: the per-layer kernels' tile wherever it is legal for the layer") \
    X(target_wgs,          "MPDX_TARGET_WGS",           INT,     160,     ONCE, "choose_tile takes the largest tile that still gives this many workgroups (160 of the 256 CUs)") \
    X(lds_cap_kb,          "MPDX_LDS_CAP_KB",           INT,     96,      ONCE, "choose_tile's LDS budget per workgroup in KiB (<= 96 so that a second workgroup can co-reside)") \
    X(ksplit,              "MPDX_KSPLIT",               INT,     -1,      ONCE, "k5 GroupNorm layers: 0 = (NT/16) x (8/(NT/16)) waves, 1 = 1 x 8 (K split), -1 by the layer's K") \
    X(wsn_min_b,           "MPDX_WSN_MIN_B",            INT,     512,     ONCE, "smallest batch for conv_wsn_kernel (profiles/r05_wsn_threshold_sweep.txt)") \
    X(wsp_min_b,           "MPDX_WSP_MIN_B",            INT,     512,     ONCE, "smallest batch for conv_wsp_kernel (same sweep)") \
    X(ws_ns,               "MPDX_WS_NS",                INT,     0,       ONCE, "256 -> 256 weight-stationary kernel: 1 / 2 force one / two 32-position tiles per step, 0 by batch") \
    /* ---- training: development A/B knobs, each decided; the default is the winner */ \
    X(train_deferred,      "MPDX_TRAIN_DEFERRED",       ON,      true,    ONCE, "0: weight-gradient partial sums reduced per layer, not deferred to one reduction at the end of the pass") \
    X(train_restream_ride, "MPDX_TRAIN_RESTREAM_RIDE",  ON,      true,    ONCE, "0: the fused programs' weight streams are re-assembled by a launch of their own, not by side blocks of time_train_fwd_kernel") \
    X(train_gn_fuse,       "MPDX_TRAIN_GN_FUSE",        ON,      true,    ONCE, "0: Mish + GroupNorm backward as its own launch, not the epilogue of the consumer's input-gradient convolution") \
    X(train_bwd_prog,      "MPDX_TRAIN_BWD_PROG",       INT,     1,       ONCE, "whole-trajectory backward programs of the outer levels (fused_bwd.hpp): 0 off, 2 the down program only") \
    X(train_bwd_prog_max_b,"MPDX_TRAIN_BWD_PROG_MAX_B", INT,     512,     ONCE, "largest batch that runs the backward programs") \
    X(wgrad_late_div,      "MPDX_WGRAD_LATE_DIV",       INT,     kUnset,  ONCE, "divisor (>= 1) of the batch splits of the weight gradients that run behind the chain and of the backward programs'; unset: 4 / 8 / 4 at batch < 64 / <= 128 / beyond (profiles/r06_train_late_div_ab.txt)") \
    X(wgrad_prog_mul,      "MPDX_WGRAD_PROG_MUL",       INT,     1,       ONCE, "batch < 64: split multiplier (<= 4) of the backward programs' weight gradients (2: 0.513 against 0.49 ms, profiles/r06_train_b32_split_ab.txt)") \
    X(train_wgrad_late,    "MPDX_TRAIN_WGRAD_LATE",     INT,     -1,      ONCE, "weight gradients leave the chain and run behind it in one launch: 0 / 1 force, -1 from batch 48 on (batch 32 no gain, 48 0.58 -> 0.543 ms, 128 -3 %, 512 -4.6 %)") \
    X(train_wgrad_multi,   "MPDX_TRAIN_WGRAD_MULTI",    ON,      true,    ONCE, "0: the late weight-gradient jobs three per launch, not all in one wgrad_multi_kernel launch") \
    X(train_reduce_join,   "MPDX_TRAIN_REDUCE_JOIN",    ON,      true,    ONCE, "0: the column sums as their own launch, not side blocks of the weight-gradient reduction's") \
    X(time_tail_split,     "MPDX_TIME_TAIL_SPLIT",      ON,      true,    ONCE, "0: the time encoder's backward tail inside time_bwd_all_kernel, not as time_tail_kernel's 8 blocks behind it")
// clang-format on

// ---- the parse kinds: C++ type, and value from getenv's result `e` (null: not set) and the row's default
using PRESENT_t = bool;
using ON_t = bool;
using INT_t = int;
using UINT_t = unsigned;
using STR_t = const char*;
inline bool parse_PRESENT(const char* e, bool) { return e != nullptr; }
inline bool parse_ON(const char* e, bool) { return !(e && atoi(e) == 0); }
inline int parse_INT(const char* e, int dflt) { return e ? atoi(e) : dflt; }
inline unsigned parse_UINT(const char* e, unsigned dflt) { return e ? (unsigned)strtoul(e, nullptr, 0) : dflt; }
inline const char* parse_STR(const char* e, const char*) { return e; }

// ---- the accessors: sw::debug(), sw::debug_fuse(), ...
#define MPDX_SW_READ_ONCE(T, expr) static const T v = (expr); return v;
#define MPDX_SW_READ_LIVE(T, expr) return (expr);
#define MPDX_SW_ACCESSOR(fn, NAME, KIND, DFLT, TIMING, DOC) \
    inline KIND##_t fn() { MPDX_SW_READ_##TIMING(KIND##_t, parse_##KIND(std::getenv(NAME), DFLT)) }
MPDX_SWITCHES(MPDX_SW_ACCESSOR)
#undef MPDX_SW_ACCESSOR
#undef MPDX_SW_READ_ONCE
#undef MPDX_SW_READ_LIVE

}  // namespace sw
}  // namespace mpdx
