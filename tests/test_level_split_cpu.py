"""Host side of the paired joined launch, without a device: the launch geometry the kernel and the host share (csrc/fused_level.hpp split_slot /
split_block / split_grid, through mpdx_level_split_block) for every batch the launch admits, and the option of a handle."""
import ctypes as C

import pytest

CUS = 256


@pytest.fixture(scope="module")
def lib():
    from mpd_public_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_grid_covers_every_trajectory_role_once_on_one_xcd(lib):
    """For B = 1 .. 128: the grid is 2 x 8 ceil(B / 8) blocks and resident at one workgroup per compute unit, it holds each (trajectory, role) exactly
    once, block x < nb8 is the primary of trajectory x and block x + nb8 its helper, both share block % 8 (workgroups are dealt round-robin over the
    8 XCDs), and exactly the blocks of trajectories >= B are named surplus (they leave at once)."""
    b, r = C.c_int32(), C.c_int32()
    for B in range(1, 129):
        nb8 = 8 * -(-B // 8)
        grid = lib.mpdx_level_split_block(B, 0, C.byref(b), C.byref(r))
        assert grid == 2 * nb8 and grid <= CUS, (B, grid)
        seen, xcd, surplus = set(), {}, []
        for x in range(grid):
            assert lib.mpdx_level_split_block(B, x, C.byref(b), C.byref(r)) == grid
            assert r.value == (0 if x < nb8 else 1), (B, x)
            if b.value < 0:
                surplus.append(x)
                continue
            assert b.value == x - r.value * nb8 and b.value < B and (b.value, r.value) not in seen
            seen.add((b.value, r.value))
            assert xcd.setdefault(b.value, x % 8) == x % 8 == b.value % 8, (B, x)
        assert len(seen) == 2 * B, B
        assert surplus == [x for x in range(grid) if x % nb8 >= B], B


def test_block_map_refuses_what_it_cannot_answer(lib):
    assert lib.mpdx_level_split_block(0, 0, None, None) < 0
    assert lib.mpdx_level_split_block(129, 0, None, None) < 0 and b"B=129" in lib.mpdx_last_error()   # 2 x 136 blocks: never admitted
    assert lib.mpdx_level_split_block(3, 16, None, None) < 0    # B = 3: nb8 = 8, 16 blocks
    assert lib.mpdx_level_split_block(3, -1, None, None) < 0
    assert lib.mpdx_level_split_block(3, 15, None, None) == 16


def test_option_of_a_handle(lib):
    from mpd_public_amd import _lib
    cfg = _lib.UnetCfg(4, 64, 32, 4, (C.c_int32 * _lib.MAX_LEVELS)(1, 2, 4, 8), 32)
    h = C.c_void_p()
    assert lib.mpdx_unet_create(C.byref(cfg), C.byref(h)) == 0
    for on in (0, 1, -1, 5):
        assert lib.mpdx_unet_set_level_split(h, on) == 0
    assert lib.mpdx_unet_plan_split(h) == 0                      # no plan yet
    assert lib.mpdx_unet_set_level_split(None, 1) < 0
    assert lib.mpdx_unet_plan_split(None) == 0
    lib.mpdx_unet_destroy(h)
