"""Density-only coarse evaluations (csrc/nwe_mfma_eval.h: mlp_eval, density_only).

A lean frame (rgb / depth / acc only) with importance sampling reads nothing of the coarse pass but its weights, which depend
on sigma alone, so its LEAN kernel ends every coarse evaluation with the trunk and skips the view layer and the rgb head.  Any
further output selects the full instantiation, which keeps computing the coarse colour: the two must agree bit for bit on
every output the lean frame has, for every work decomposition, sample setting and ragged ray count.  A frame without
importance sampling (the coarse colour IS the output) must not take the density-only path at all, and neither does a 6-deep
network, whose gamma(x) skip input enters the last trunk layer (density_only_built): its lean frames keep the coarse colour.
"""
import numpy as np
import pytest
import torch

import nwe_amd
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

LEAN = ("rgb", "depth", "acc")
FULL = ("rgb", "depth", "acc", "rgb_coarse")
FLAG_RGB_COARSE = 1 << 4
FLAGS_KEPT = 0x7 | 0xE0   # bits 0-2 (fine rgb / depth / acc) and 5-7 (coarse depth / acc / disp)


def _renderer(D, W, seed=2000, coarse=None):
    r = nwe_amd.Renderer(0)
    r.set_network(0, coarse if coarse is not None else nwe_amd.synthetic.make_state_dict(seed, D, W))
    r.set_network(1, nwe_amd.synthetic.make_state_dict(seed + 1, D, W))
    return r


def _frame(r, H, W, precision, outputs):
    fx, fy, cx, cy = O.intrinsics(H, W)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    return r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, precision=precision, outputs=outputs)


def _assert_lean_equals_full(lean, full, ctx):
    for k in LEAN:
        assert torch.equal(lean[k], full[k]), (ctx, k)
    fl, ff = int(lean["flags"].item()), int(full["flags"].item())
    assert fl & FLAGS_KEPT == ff & FLAGS_KEPT, (ctx, hex(fl), hex(ff))
    return fl, ff


@pytest.mark.parametrize("D,W", [(8, 256), (4, 128), (6, 256), (6, 128)])
def test_lean_frame_equals_full_frame(D, W):
    """Folded 8x256 and 4x128 (density-only coarse pass) and 6x256, 6x128 (full coarse pass), both MFMA modes, ns in {64, 37} x ni in {128, 17}, decompositions 0 / 1 / 2, a ragged ray count
    (13 x 29 = 377 rays: neither packets nor workgroups come out even)."""
    r = _renderer(D, W)
    try:
        for ns, ni in ((64, 128), (37, 17), (64, 17), (37, 128)):
            r.set_sampling(ns, ni)
            for mode in (0, 1, 2):
                r.debug_set_decomposition(mode)
                for precision in ("f16x3", "f16x1"):
                    ctx = (D, W, ns, ni, mode, precision)
                    lean = _frame(r, 13, 29, precision, LEAN)
                    full = _frame(r, 13, 29, precision, FULL)
                    fl, _ = _assert_lean_equals_full(lean, full, ctx)
                    assert not fl & FLAG_RGB_COARSE, ctx
    finally:
        r.debug_set_decomposition(-1)
        r.close()


def test_lean_frame_equals_full_frame_both_hybrid_launches():
    """The hybrid plan (the one the benchmark frame takes) on 300 x 200 = 60000 rays at 8x256, 64 + 128 samples: one full round
    of packet workgroups plus a sample-split rest, both launches in their LEAN instantiation; and the launcher's own choice."""
    r = _renderer(8, 256)
    try:
        r.set_sampling(64, 128)
        for mode in (2, -1):
            r.debug_set_decomposition(mode)
            lean = _frame(r, 200, 300, "f16x3", LEAN)
            assert mode == -1 or r.debug_last_plan() == 2
            full = _frame(r, 200, 300, "f16x3", FULL)
            _assert_lean_equals_full(lean, full, mode)
    finally:
        r.debug_set_decomposition(-1)
        r.close()


@pytest.mark.parametrize("D,density_only", [(8, True), (6, False)])
def test_coarse_colour_flag_is_not_raised_in_lean_frames(D, density_only):
    """A coarse network whose rgb head yields NaN: the full frame reports the NaN coarse colour (bit 4); a lean frame with a
    density-only coarse pass has no coarse colour to report, a 6-deep one still computes and reports it.  Every output and
    every other flag bit is the same in both frames."""
    sd = nwe_amd.synthetic.make_state_dict(2000, D, 256)
    sd["_rgb_linear.bias"] = np.full_like(sd["_rgb_linear.bias"], np.nan)
    r = _renderer(D, 256, coarse=sd)
    try:
        r.set_sampling(64, 128)
        for mode in (0, 1):
            r.debug_set_decomposition(mode)
            lean = _frame(r, 13, 29, "f16x3", LEAN)
            full = _frame(r, 13, 29, "f16x3", FULL)
            fl, ff = _assert_lean_equals_full(lean, full, mode)
            assert ff & FLAG_RGB_COARSE and bool(fl & FLAG_RGB_COARSE) != density_only, (mode, hex(fl), hex(ff))
            assert torch.isfinite(lean["rgb"]).all()
    finally:
        r.debug_set_decomposition(-1)
        r.close()


@pytest.mark.parametrize("D,W", [(8, 256), (4, 128), (6, 256)])
def test_lean_frame_without_importance_sampling_keeps_coarse_colour(D, W):
    """ni = 0: the coarse pass is the frame, its colour the output - the lean frame runs full coarse evaluations."""
    r = _renderer(D, W)
    try:
        r.set_sampling(37, 0)
        for mode in (0, 1):
            r.debug_set_decomposition(mode)
            for precision in ("f16x3", "f16x1"):
                lean = _frame(r, 13, 29, precision, LEAN)
                full = _frame(r, 13, 29, precision, FULL)
                _assert_lean_equals_full(lean, full, (D, W, mode, precision))
                assert torch.equal(full["rgb_coarse"], full["rgb"])
                assert float(lean["rgb"].std()) > 0.0   # a real colour, not the density-only zeros
    finally:
        r.debug_set_decomposition(-1)
        r.close()
