"""Packets of 8x4 pixel blocks without a GPU (csrc/nwe_packet_blocks.h, csrc/nwe_plan.cpp; include/nwe.h:
nwe_debug_set_packet_blocks).  The map from ray index to pixel is the function the kernels compile, reached through
nwe_debug_packet_pixels; the planner's decision is read with nwe_debug_last_packet_blocks behind nwe_debug_plan on a host-only
context, the way tests/test_plan_host.py drives the planner."""
import ctypes as C

import numpy as np
import pytest

import nwe_amd
from nwe_amd import _lib, synthetic

CASES = [(P, R, W) for P in (1, 3) for R in (4, 8, 200) for W in (8, 24, 800)]


def _pixels(n, W, first=0):
    out = np.empty(n, dtype=np.int32)
    assert _lib.load().nwe_debug_packet_pixels(first, n, W, out.ctypes.data) == _lib.NWE_OK
    return out.astype(np.int64)


@pytest.mark.parametrize("P,R,W", CASES)
def test_the_map_is_a_bijection_and_every_packet_is_one_block(P, R, W):
    n = P * R * W
    pix = _pixels(n, W)
    assert np.array_equal(np.sort(pix), np.arange(n))
    # the formula of the header, restated
    j = np.arange(n)
    r = j % (4 * W)
    want = j - r + (r % 32 // 8) * W + r // 32 * 8 + r % 8
    assert np.array_equal(pix, want)
    # every aligned group of 32 indices: one pose, 4 consecutive rows from a multiple of 4, 8 consecutive columns from a multiple
    # of 8, each pixel of the block once, row-major inside the block
    g = pix.reshape(-1, 32)
    pose, row, col = g // (R * W), g % (R * W) // W, g % W
    assert (pose == pose[:, :1]).all()
    assert (row[:, 0] % 4 == 0).all() and (col[:, 0] % 8 == 0).all()
    k = np.arange(32)
    assert (row == row[:, :1] + k // 8).all() and (col == col[:, :1] + k % 8).all()
    # a window of the map is the map
    assert np.array_equal(_pixels(min(n, 96), W, first=n - min(n, 96)), pix[n - min(n, 96):])


def test_the_entry_point_checks_its_arguments():
    lib = _lib.load()
    out = np.empty(4, dtype=np.int32)
    assert lib.nwe_debug_packet_pixels(0, 4, 8, None) == _lib.NWE_ERR_INVALID
    assert lib.nwe_debug_packet_pixels(-1, 4, 8, out.ctypes.data) == _lib.NWE_ERR_INVALID
    assert lib.nwe_debug_packet_pixels(0, -1, 8, out.ctypes.data) == _lib.NWE_ERR_INVALID
    assert lib.nwe_debug_packet_pixels(0, 4, 0, out.ctypes.data) == _lib.NWE_ERR_INVALID
    assert lib.nwe_debug_packet_pixels((1 << 31) - 2, 4, 8, out.ctypes.data) == _lib.NWE_ERR_INVALID
    assert lib.nwe_debug_packet_pixels(0, 0, 8, None) == _lib.NWE_OK
    assert lib.nwe_debug_last_packet_blocks(None) == -1 and lib.nwe_debug_set_packet_blocks(None, 1) == _lib.NWE_ERR_INVALID


def _renderer(monkeypatch, env=None, ns=8, ni=8):
    monkeypatch.delenv("NWE_PACKET_BLOCKS", raising=False)
    if env is not None:
        monkeypatch.setenv("NWE_PACKET_BLOCKS", env)
    r = nwe_amd.Renderer(host_only=True)
    for which in (0, 1):
        r.set_network(which, synthetic.make_state_dict(1000 + which, D=4, W=128))
    r.set_sampling(ns, ni)
    return r


def _blocked(r, P=1, H=64, W=64, rows=None, outputs=("rgb", "depth", "acc"), precision=_lib.PREC_F16X3, n_rays=-1, cus=256):
    """nwe_debug_plan of the call, then what the planner said about its packets."""
    r0, r1 = (0, H) if rows is None else rows
    out = _lib.Outputs(**{k: 1 for k in outputs})
    rc = _lib.load().nwe_debug_plan(r._ctx, P, H, W, r0, r1, n_rays, C.byref(out), 0, precision, cus, C.byref(_lib.PlanReport()))
    assert rc == _lib.NWE_OK, _lib.load().nwe_last_error(r._ctx).decode()
    return r.debug_last_packet_blocks()


def test_the_planner_blocks_exactly_the_calls_that_fit(monkeypatch):
    r = _renderer(monkeypatch)
    try:
        assert r.debug_last_packet_blocks() == 0                      # nothing planned yet
        for P, R, W in CASES:
            for cus in (8, 256):
                assert _blocked(r, P, 256, W, rows=(8, 8 + R), cus=cus) == 1, (P, R, W, cus)
        for dec in (0, 1, 2):                                         # every decomposition; precision f16x1 as well
            r.debug_set_decomposition(dec)
            assert _blocked(r) == 1 and _blocked(r, precision=_lib.PREC_F16X1) == 1, dec
        r.debug_set_decomposition(-1)
        assert _blocked(r, rows=(5, 9)) == 1                          # 4 rows from any first row: bands are the call's, not the image's
        # rows that are no multiple of 4, a width that is no multiple of 8
        for rows in ((0, 3), (0, 6), (0, 75), (5, 11)):
            assert _blocked(r, H=128, rows=rows) == 0, rows
        assert _blocked(r, W=12) == 0 and _blocked(r, H=6, W=12) == 0
        assert _blocked(r) == 1                                       # ... and the answer is the last call's, not a latch
        # ray lists, outputs beyond the lean ones, the fp32 kernel
        assert _blocked(r, n_rays=64 * 64) == 0
        assert _blocked(r, outputs=("rgb", "z_fine")) == 0 and _blocked(r, outputs=("rgb", "disp")) == 0
        assert _blocked(r, precision=_lib.PREC_F32) == 0
        # the modes with kernels of their own
        r.set_early_termination(0.01)
        assert _blocked(r) == 0
        r.set_early_termination(0.0)
        r.set_shared_coarse(2)
        assert _blocked(r) == 0
        r.set_shared_coarse(1)
        r.set_separate_passes(True)
        assert _blocked(r) == 0
        r.set_separate_passes(False)
        r.set_occupancy(np.ones((4, 4, 4), dtype=bool), (-1, -1, -1), (1, 1, 1), 4)
        assert _blocked(r) == 0
        r.clear_occupancy()
        r.set_coarse_grid(np.zeros((4, 4, 4), dtype=np.float32), (-1, -1, -1), (1, 1, 1))
        assert _blocked(r) == 0
        r.clear_coarse_grid()
        assert _blocked(r) == 1
        # a single pass (no importance samples) is a lean plain call like any other
        r.set_sampling(8, 0)
        assert _blocked(r) == 1
        r.set_sampling(8, 8)
        # the switch
        r.debug_set_packet_blocks(False)
        assert _blocked(r) == 0
        r.debug_set_packet_blocks(True)
        assert _blocked(r) == 1
        for bad in (-1, 2):
            assert _lib.load().nwe_debug_set_packet_blocks(r._ctx, bad) == _lib.NWE_ERR_INVALID and _blocked(r) == 1
    finally:
        r.close()
    # the unfolded formulation has the plain kernels (and no hollow path): blocked all the same, nothing depends on it
    r = _renderer(monkeypatch)
    try:
        r.debug_set_fold(False)
        for which in (0, 1):
            r.set_network(which, synthetic.make_state_dict(1000 + which, D=4, W=128))
        assert _blocked(r) == 1
    finally:
        r.close()


def test_the_environment_sets_what_a_new_context_starts_with(monkeypatch):
    for env, want in ((None, 1), ("1", 1), ("0", 0), ("junk", 1)):
        r = _renderer(monkeypatch, env)
        try:
            assert _blocked(r) == want, env
            r.debug_set_packet_blocks(True)
            assert _blocked(r) == 1
        finally:
            r.close()
