"""The work queue without a GPU (include/nwe.h: nwe_debug_set_work_queue): the setter's domain and default on a host-only
context, the environment variable a new context takes its mode from, and the grid of a queued launch."""
import ctypes as C

import pytest

import nwe_amd
from nwe_amd import _lib


def test_default_setter_domain_and_getter_on_a_host_only_context(monkeypatch):
    monkeypatch.delenv("NWE_WORK_QUEUE", raising=False)
    r = nwe_amd.Renderer(host_only=True)
    lib = _lib.load()
    try:
        assert r.debug_get_work_queue() == -1                              # queue a launch larger than the device
        for mode in (0, 1, -1):
            r.debug_set_work_queue(mode)
            assert r.debug_get_work_queue() == mode
        r.debug_set_work_queue(1)
        for bad in (2, -2, 3, 256, -(1 << 20)):
            assert lib.nwe_debug_set_work_queue(r._ctx, bad) == _lib.NWE_ERR_INVALID
            with pytest.raises(ValueError):
                r.debug_set_work_queue(bad)
            assert r.debug_get_work_queue() == 1                           # the previous value stays
        assert lib.nwe_debug_set_work_queue(None, 0) == _lib.NWE_ERR_INVALID and lib.nwe_debug_get_work_queue(None) == -2
        # nothing was launched on a host-only context
        items, grid, taken, side = (C.c_uint * 2)(7, 7), (C.c_uint * 2)(7, 7), (C.c_uint * 2)(7, 7), C.c_int(7)
        assert lib.nwe_debug_last_queue(r._ctx, items, grid, taken, C.byref(side)) == _lib.NWE_ERR_STATE
        assert (list(items), list(grid), list(taken), side.value) == ([0, 0], [0, 0], [0, 0], 0)
        assert lib.nwe_debug_last_queue(r._ctx, None, grid, taken, None) == _lib.NWE_ERR_INVALID
    finally:
        r.close()


@pytest.mark.parametrize("text, mode", [("0", 0), ("1", 1), ("", -1), ("2", -1), ("-1", -1), ("01", -1), ("on", -1)])
def test_environment_sets_the_default_of_a_new_context_and_the_setter_wins(monkeypatch, text, mode):
    first = nwe_amd.Renderer(host_only=True)            # created before the variable is set: keeps its own default
    monkeypatch.setenv("NWE_WORK_QUEUE", text)
    r = nwe_amd.Renderer(host_only=True)
    try:
        assert r.debug_get_work_queue() == mode          # anything but "0" / "1" is ignored
        assert first.debug_get_work_queue() == -1
        for m in (1, 0, -1):
            r.debug_set_work_queue(m)
            assert r.debug_get_work_queue() == m         # the setter overrides the environment
        monkeypatch.delenv("NWE_WORK_QUEUE")
        assert r.debug_get_work_queue() == -1 and nwe_amd.Renderer(host_only=True).debug_get_work_queue() == -1
    finally:
        r.close(); first.close()


def test_grid_of_a_queued_launch():
    """n work items -> n plus a quarter (rounded up), rounded up to a multiple of 8: every XCD's eighth of the grid holds at
    least 1.25 x its eighth of the items."""
    grid = _lib.load().nwe_debug_queue_grid
    assert [grid(n) for n in (0, 1, 2, 3, 4, 5, 6, 7, 8, 24, 32, 64)] == [0, 8, 8, 8, 8, 8, 8, 16, 16, 32, 40, 80]
    assert grid(4864) == 6080 and grid(544) == 680      # the two launches of the 800 x 800 frame
    assert grid(469) == 592                             # 60000 rays as packets: 469 + 118 = 587 -> 592
    for n in list(range(1, 600)) + [4864, 20000, 67108863]:
        g = grid(n)
        assert g % 8 == 0 and g >= n + (n + 3) // 4 and g - 8 < n + (n + 3) // 4, n
    assert grid(67108864) == 83886080                   # 2^31 rays in 32-ray items: no 32-bit overflow on the way


@pytest.mark.parametrize("text, backfill", [("0", 0), ("1", 1), ("", 1), ("00", 1), ("no", 1)])
def test_backfill_variable_of_a_new_context(monkeypatch, text, backfill):
    """NWE_WORK_QUEUE_BACKFILL=0 keeps a new context's second launch behind the first (the A/B arm of tools/ab_bench.sh); anything
    else, and no variable, leaves the backfill on.  It does not touch the mode."""
    lib = _lib.load()
    monkeypatch.delenv("NWE_WORK_QUEUE", raising=False)
    monkeypatch.delenv("NWE_WORK_QUEUE_BACKFILL", raising=False)
    first = nwe_amd.Renderer(host_only=True)
    monkeypatch.setenv("NWE_WORK_QUEUE_BACKFILL", text)
    r = nwe_amd.Renderer(host_only=True)
    try:
        assert lib.nwe_debug_get_work_queue_backfill(r._ctx) == backfill and r.debug_get_work_queue() == -1
        assert lib.nwe_debug_get_work_queue_backfill(first._ctx) == 1
        assert lib.nwe_debug_get_work_queue_backfill(None) == -1
    finally:
        r.close(); first.close()
