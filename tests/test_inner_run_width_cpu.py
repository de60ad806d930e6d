"""Host side of the runs' width, without a device: the launch geometry the kernel and the host share (csrc/inner_run.hpp run_slot / run_block /
run_grid, through mpdx_inner_run_block) for every batch the runs admit at both widths, and the width option of a handle."""
import ctypes as C

import pytest

CUS = 256


@pytest.fixture(scope="module")
def lib():
    from mpd_public_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("width", [16, 32])
def test_grid_covers_every_cluster_tile_once_on_one_xcd(lib, width):
    """For B = 1 .. 128: the grid holds each (cluster, channel tile) exactly once, the surplus blocks leave, a cluster's 8 blocks share block % 8
    (workgroups are dealt round-robin over the 8 XCDs), the grid is resident (two workgroups per compute unit at width 16, one at 32) and the counter
    area holds a line per cluster."""
    c, m, lines = C.c_int32(), C.c_int32(), C.c_int32()
    for B in range(1, 129):
        nc = -(-B // (width // 8))
        grid = lib.mpdx_inner_run_block(B, width, CUS, 0, C.byref(c), C.byref(m), C.byref(lines))
        assert grid == -(-nc // 8) * 64 and grid <= CUS * (2 if width == 16 else 1), (B, grid)
        assert lines.value >= nc, (B, lines.value)
        seen, xcd = set(), {}
        for b in range(grid):
            assert lib.mpdx_inner_run_block(B, width, CUS, b, C.byref(c), C.byref(m), None) == grid
            assert 0 <= m.value < 8
            if c.value < 0:
                continue
            assert c.value < nc and (c.value, m.value) not in seen
            seen.add((c.value, m.value))
            assert xcd.setdefault(c.value, b % 8) == b % 8, (B, b)
        assert len(seen) == 8 * nc, B
    assert lines.value == (72 if width == 16 else 40)


def test_block_map_refuses_what_it_cannot_answer(lib):
    assert lib.mpdx_inner_run_block(4, 8, CUS, 0, None, None, None) < 0      # no such width
    assert lib.mpdx_inner_run_block(0, 16, CUS, 0, None, None, None) < 0
    assert lib.mpdx_inner_run_block(4, 16, CUS, 64, None, None, None) < 0    # B = 4 at width 16: one group of 8 clusters, 64 blocks
    assert lib.mpdx_inner_run_block(4, 16, CUS, 63, None, None, None) == 64


def test_width_option_of_a_handle(lib):
    from mpd_public_amd import _lib
    cfg = _lib.UnetCfg(4, 64, 32, 4, (C.c_int32 * _lib.MAX_LEVELS)(1, 2, 4, 8), 32)
    h = C.c_void_p()
    assert lib.mpdx_unet_create(C.byref(cfg), C.byref(h)) == 0
    for w in (16, 32, 0):
        assert lib.mpdx_unet_set_inner_run_width(h, w) == 0
    for bad in (-1, 8, 64, 4):
        assert lib.mpdx_unet_set_inner_run_width(h, bad) < 0 and b"width" in lib.mpdx_last_error()
    assert lib.mpdx_unet_set_inner_run_width(None, 16) < 0
    assert lib.mpdx_unet_set_inner_run_parts(h, 4) < 0                        # the width is no part
    lib.mpdx_unet_destroy(h)
