#!/usr/bin/env python3
"""Cycle stamps of the paired joined launch (fused_join_split_kernel), trajectory 0, all 4 waves of the primary and of the helper (dev tool, needs a GPU
and a -DMPDX_DEV_HOOKS library in MPDX_LIB).  Prints the level's ops 10 - 14 per role: k-loop, epilogue, publish (drain + barrier + add), poll wait, load
of the partner's half + barrier; and the helper's entry.  With the option off (argument 2 = 0) the unpaired kernel's ops 10 - 14 as far as its stamps reach."""
import ctypes as C, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import torch
from bench import build_model
from mpd_public_amd import _lib
B = int(sys.argv[1]) if len(sys.argv) > 1 else 100
on = int(sys.argv[2]) if len(sys.argv) > 2 else 1
dm, sd = build_model(4, (1, 2, 4, 8), 100, "cuda")
lib = _lib.load()
hdl, packed, tab, ws = dm.model.engine(100, B)
dm.model.set_level_split(bool(on))
x = torch.randn(B, 64, 4, device="cuda")
dm.model(x, torch.full((B,), 50, device="cuda", dtype=torch.long))
st = torch.cuda.current_stream().cuda_stream
for seg in range(8):
    stamps = (C.c_longlong * 1024)(); n = C.c_int(); nops = C.c_int()
    if lib.mpdx_fused_trace(hdl, packed.data_ptr(), tab.data_ptr(), x.data_ptr(), seg, B, ws.data_ptr(), st, stamps, 1024, C.byref(n), C.byref(nops)):
        break
    if nops.value <= 16:
        continue   # not the joined launch
    for rep in range(2):   # (the second call's stamps: warm instruction cache)
        _lib.check(lib.mpdx_fused_trace(hdl, packed.data_ptr(), tab.data_ptr(), x.data_ptr(), seg, B, ws.data_ptr(), st, stamps, 1024, C.byref(n), C.byref(nops)))
    P = [[stamps[w * 128 + i] for i in range(128) if stamps[w * 128 + i]] for w in range(4)]
    t0 = min(w[0] for w in P)
    print(f"joined launch, B = {B}, level split {'on' if on else 'off'}: primary wave 0 entry -> last stamp of its first 128: {P[0][-1] - t0} ticks")
    if not on:
        # up part 4 + 11 * 5 + 2 = 61 stamps, then five per down op: op 10 starts at 61 + 50
        names = ["entered", "k-loop", "stats", "epilogue", "barrier"]
        for oi in range(10, 14):
            for k, nm in enumerate(names):
                i = 61 + 5 * oi + k
                print(f"  down op{oi} {nm:>10s}: " + " ".join(f"{(w[i] - t0) if i < len(w) else -1:7d}" for w in P))
        break
    R = [[[stamps[512 + (r * 4 + w) * 64 + i] for i in range(64) if stamps[512 + (r * 4 + w) * 64 + i]] for w in range(4)] for r in range(2)]
    head = [["op9 done", "entry published", "level start"], ["helper entry", "requests issued", "slot 0 seen", "level start"]]
    per = ["entered", "k-loop", "stats", "epilogue", "published", "partner seen", "loaded"]
    last = ["entered", "k-loop", "bias", "epilogue", "barrier"]
    for r in range(2):
        names = list(head[r])
        for oi in range(10, 14):
            names += [f"op{oi} {p}" for p in per]
        names += [f"op14 {p}" for p in last]
        print(f"  role {r} ({'primary' if r == 0 else 'helper'}), ticks since the primary's entry, waves 0-3")
        for i, nm in enumerate(names):
            print(f"  {nm:>22s}: " + " ".join(f"{(w[i] - t0) if i < len(w) else -1:7d}" for w in R[r]))
    # the hand-off of an op as the slower role sees it: epilogue done -> loaded
    for oi in range(4):
        base = [3, 4]
        h = [max(R[r][w][base[r] + 7 * oi + 6] - R[r][w][base[r] + 7 * oi + 3] for w in range(4)) for r in range(2)]
        k = [max(R[r][w][base[r] + 7 * oi + 1] - R[r][w][base[r] + 7 * oi + 0] for w in range(4)) for r in range(2)]
        pub = [max(R[r][w][base[r] + 7 * oi + 4] - R[r][w][base[r] + 7 * oi + 3] for w in range(4)) for r in range(2)]
        poll = [R[r][0][base[r] + 7 * oi + 5] - R[r][0][base[r] + 7 * oi + 4] for r in range(2)]
        load = [max(R[r][w][base[r] + 7 * oi + 6] - R[r][w][base[r] + 7 * oi + 5] for w in range(4)) for r in range(2)]
        print(f"  op{10 + oi}: k-loop {k}, epilogue-done -> loaded {h} (publish {pub}, poll {poll}, load + barrier {load}) ticks [primary, helper]")
    break
