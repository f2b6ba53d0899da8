"""CPU-side checks of cvae_safety_metrics (no GPU calls): every host validation returns
CVAE_E_INVALID with its message before anything is launched — the device pointers here are NULL,
so a launch would not get that far — and the legal empty population returns OK."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def cl():
    from cvae_amd import _build, _lib, safety  # noqa: F401  (the module under test must import)
    _build.build()
    return _lib


def call(cl, scene=0, want_rows=0, block_waves=0, merge=1, log_off=(0, 10), flags=(3,), n_log_rows=10,
         off=(0, 4), n_state_rows=4, lot=(0,)):
    cfg = cl.CvaeSafetyConfig()
    cfg.scene, cfg.want_rows, cfg.block_waves, cfg.merge = scene, want_rows, block_waves, merge
    lo, fl = np.asarray(log_off, np.int64), np.asarray(flags, np.int32)
    of, lt = np.asarray(off, np.int64), np.asarray(lot, np.int32)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = cl.lib().cvae_safety_metrics(C.byref(cfg), None, n_log_rows, None, hp(lo), len(lo) - 1, None, hp(fl), None,
                                      n_state_rows, None, hp(of), len(lt), None, hp(lt), None, None, None, 0, None)
    return cl.check(rc, "cvae_safety_metrics")


@pytest.mark.parametrize("kw,msg", [
    (dict(scene=4), "bad scene"),
    (dict(block_waves=9), "bad safety parameter"),
    (dict(want_rows=4), "bad safety parameter"),
    (dict(log_off=(0, 6, 5, 10), flags=(3, 3, 3)), "log offsets must be monotone"),
    (dict(log_off=(0, 9)), "log offsets must end at n_log_rows"),
    (dict(off=(0, 5, 4), lot=(0, 0)), "row offsets must be monotone"),
    (dict(off=(0, 3)), "row offsets must end at n_rows"),
    (dict(lot=(1,)), "log_of_track outside the logs"),
    (dict(lot=(-1,)), "log_of_track outside the logs"),
    (dict(flags=(1,)), "no finite ego_x/ego_y row"),
])
def test_invalid_input_is_refused_before_the_launch(cl, kw, msg):
    with pytest.raises(cl.CvaeError, match=msg):
        call(cl, **kw)


def test_valid_tables_reach_the_pointer_check(cl):
    """the same tables pass validation: the next refusal is the NULL device pointer, still no launch"""
    with pytest.raises(cl.CvaeError, match="null argument"):
        call(cl)


def test_empty_population_is_legal(cl):
    assert call(cl, off=(0,), n_state_rows=0, lot=()) == 0
    assert call(cl, merge=0, lot=()) == 0
    # an empty track or an empty log needs no finite row: validation passes (then the NULL pointers)
    with pytest.raises(cl.CvaeError, match="null argument"):
        call(cl, flags=(1,), off=(0, 0), n_state_rows=0)
    with pytest.raises(cl.CvaeError, match="null argument"):
        call(cl, log_off=(0, 0), flags=(0,), n_log_rows=0)
