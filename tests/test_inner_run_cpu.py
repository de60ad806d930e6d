"""Host side of the inner-level run's error path, without a device: the handle's sticky status word - what a workgroup that gives up its bounded
wait sets - turns into MPDX_E_DEVICE from mpdx_unet_status and mpdx_plan, and clearing it lets the handle go on."""
import ctypes as C

import pytest

E_STATE, E_DEVICE = -3, -4


@pytest.fixture(scope="module")
def lib():
    from mpd_public_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _handle(lib):
    from mpd_public_amd import _lib
    cfg = _lib.UnetCfg(4, 64, 32, 4, (C.c_int32 * _lib.MAX_LEVELS)(1, 2, 4, 8), 32)
    h = C.c_void_p()
    assert lib.mpdx_unet_create(C.byref(cfg), C.byref(h)) == 0
    return h


def _plan(lib, h):
    """mpdx_plan with pointers that are never dereferenced on the paths taken here"""
    from mpd_public_amd import _lib
    d = C.c_void_p(64)
    coefs = (_lib.StepCoefs * 4)()
    return lib.mpdx_plan(h, d, d, 4, coefs, 0, d, None, None, None, None, 4, d, None, 0, 0, None, 0, 0, 0, None)


def test_status_word_turns_into_the_error_return(lib):
    h = _handle(lib)
    assert lib.mpdx_unet_status(h) == 0 and lib.mpdx_unet_inner_runs(h) == 0
    assert _plan(lib, h) == E_STATE and b"parameters packed" in lib.mpdx_last_error()      # a healthy handle gets as far as the parameter check
    assert lib.mpdx_unet_set_status(h, 0x301) == 0                                          # as a give-up in layer 3 of the run would
    assert lib.mpdx_unet_status(h) == E_DEVICE
    msg = lib.mpdx_last_error()
    assert b"gave up" in msg and b"0x301" in msg and b"layer 3" in msg
    assert _plan(lib, h) == E_DEVICE and b"mpdx_plan" in lib.mpdx_last_error()              # refused before anything else happens
    assert lib.mpdx_unet_status(h) == E_DEVICE                                              # sticky
    assert lib.mpdx_unet_set_status(h, 0) == 0
    assert lib.mpdx_unet_status(h) == 0 and _plan(lib, h) == E_STATE
    lib.mpdx_unet_destroy(h)


def test_option_and_null_handles(lib):
    h = _handle(lib)
    assert lib.mpdx_unet_set_inner_run(h, 0) == 0 and lib.mpdx_unet_set_inner_run(h, 1) == 0
    assert lib.mpdx_unet_set_inner_run(None, 1) < 0 and lib.mpdx_unet_status(None) < 0 and lib.mpdx_unet_set_status(None, 0) < 0
    assert lib.mpdx_unet_inner_runs(None) == 0
    lib.mpdx_unet_destroy(h)
