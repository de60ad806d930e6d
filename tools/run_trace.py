#!/usr/bin/env python3
"""Per-layer cycle stamps of the two persistent runs of mpdx_plan (csrc/inner_run.hpp), workgroup 0 / thread 0 (dev tool, needs a GPU and a
-DMPDX_DEV_HOOKS build: MPDX_LIB=build_ab/libmpdx_dev.so python tools/run_trace.py [B [width]]; width 0 / 16 / 32 = set_inner_run_width).  Per layer ten stamps; printed per layer, in ticks:
the poll wait (requests issued -> predecessor published), what ran before it (entry -> requests issued: ring fill, epilogue operands, halo rows),
staging, k-loop, reduction + epilogue, publish, and the layer's total."""
import ctypes as C, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import torch
from bench import build_model
from mpd_public_amd import _lib
B = int(sys.argv[1]) if len(sys.argv) > 1 else 100
WIDTH = int(sys.argv[2]) if len(sys.argv) > 2 else 0
dm, sd = build_model(4, (1, 2, 4, 8), 100, "cuda")
lib = _lib.load()
dm.model.set_inner_run_width(WIDTH)
hdl, packed, tab, ws = dm.model.engine(100, B)
x = torch.randn(B, 64, 4, device="cuda")
dm.model(x, torch.full((B,), 50, device="cuda", dtype=torch.long))
st = torch.cuda.current_stream().cuda_stream
nseg = 0
while lib.mpdx_unet_fused_program(hdl, nseg) != -2:
    nseg += 1
SLOTS = 32
for name, seg in (("seven-layer run", nseg + 1), ("tail run", nseg + 2)):
    stamps = (C.c_longlong * 1024)(); n = C.c_int(); nl = C.c_int()
    args = (hdl, packed.data_ptr(), tab.data_ptr(), x.data_ptr(), seg, B, ws.data_ptr(), st, stamps, 1024, C.byref(n), C.byref(nl))
    _lib.check(lib.mpdx_fused_trace(*args))   # once to warm the traced path, once for the record
    _lib.check(lib.mpdx_fused_trace(*args))
    print(f"{name}, B = {B}, width {WIDTH}: {nl.value} layers; ticks of workgroup 0 / thread 0")
    print("  layer  prologue  poll-wait  staging   k-loop  red+epi  publish    total")
    for k in range(nl.value):
        s = [stamps[k * SLOTS + i] for i in range(10)]
        row = (s[1] - s[0], s[2] - s[1], s[4] - s[2], s[6] - s[4], s[8] - s[6], s[9] - s[8], s[9] - s[0])
        print(f"  {k:5d} " + " ".join(f"{v:9d}" for v in row))
    first = stamps[0]
    last = stamps[(nl.value - 1) * SLOTS + 9]
    print(f"  launch, entry of layer 0 to publish of the last layer: {last - first} ticks")
