"""Packets of 8x4 pixel blocks (csrc/nwe_packet_blocks.h; include/nwe.h: nwe_debug_set_packet_blocks).

No output depends on which 32 rays share a wave, so every comparison is torch.equal: blocks on against blocks off against the
full instantiation of the same call, which is never blocked and never takes the hollow path.  Where the path runs is predicted
from the full instantiation's own sigma (raw_fine), per 8x4 block with blocks on and per 32 consecutive rays with blocks off,
and shown by a NaN planted in the fine rgb head."""
import numpy as np
import pytest
import torch

import bench
import nwe_amd
from nwe_amd import synthetic
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.1, 10.0
LEAN = ("rgb", "depth", "acc")
FULL = LEAN + ("raw_fine",)
FLT_MAX = float(np.finfo(np.float32).max)
NETS = {"8x256": (8, 256, 0.0), "4x128": (4, 128, 0.3), "8x256-0.2": (8, 256, 0.2)}   # as tests/test_gpu_colour_skip.py: D, W, density shift


def _nets(name):
    D, W, shift = NETS[name]
    sd_c, sd_f = synthetic.make_state_dict(1000, D, W), synthetic.make_state_dict(1001, D, W)
    sd_f["_alpha_linear.bias"] = (sd_f["_alpha_linear.bias"] - np.float32(shift)).astype(np.float32)
    return sd_c, sd_f


def _renderer(sd_c, sd_f, ns=64, ni=128):
    r = nwe_amd.Renderer(0)
    r.set_network(0, sd_c)
    r.set_network(1, sd_f)
    r.set_sampling(ns, ni)
    return r


def _render(r, H, W, pose=None, rows=None, precision="f16x3", outputs=LEAN):
    """(outputs, whether the call was blocked)"""
    fx, fy, cx, cy = O.intrinsics(H, W)
    pose = np.stack([bench.sweep_pose(0, 1), bench.sweep_pose(3, 8)]) if pose is None else pose
    out = r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR, rows=rows, precision=precision, outputs=outputs)
    return out, r.debug_last_packet_blocks()


def _same(a, b, ctx, keys=LEAN + ("flags",)):
    for k in keys:
        assert torch.equal(a[k], b[k]), (ctx, k)


@pytest.mark.parametrize("net", ["8x256", "4x128"])
def test_blocks_on_equal_blocks_off_equal_the_full_instantiation(net):
    """A 64 x 64 frame under two poses (8192 rays: 64 workgroups of packets, 256 sample-split items), 64 + 128 and 37 + 17
    samples, every decomposition forced, both MFMA precisions."""
    r = _renderer(*_nets(net))
    try:
        for ns, ni in ((64, 128), (37, 17)):
            r.set_sampling(ns, ni)
            for precision in ("f16x3", "f16x1"):
                for dec in (0, 1, 2):
                    ctx = (net, ns, ni, precision, dec)
                    r.debug_set_decomposition(dec)
                    r.debug_set_packet_blocks(True)
                    on, was_on = _render(r, 64, 64, precision=precision)
                    r.debug_set_packet_blocks(False)
                    off, was_off = _render(r, 64, 64, precision=precision)
                    r.debug_set_packet_blocks(True)
                    full, was_full = _render(r, 64, 64, precision=precision, outputs=FULL)
                    assert (was_on, was_off, was_full) == (1, 0, 0), ctx
                    _same(on, off, ctx)
                    _same(on, full, ctx)
                    assert bool(torch.isfinite(on["rgb"]).all()), ctx
    finally:
        r.close()


@pytest.mark.parametrize("H,W,rows", [(6, 12, None), (64, 64, (5, 11)), (8, 12, None)], ids=["6x12", "rows-5-11-of-64x64", "8x12"])
def test_frames_that_do_not_fit_stay_linear(H, W, rows):
    r = _renderer(*_nets("4x128"))
    try:
        for dec in (0, 1):
            r.debug_set_decomposition(dec)
            lean, was = _render(r, H, W, rows=rows)
            full, was_full = _render(r, H, W, rows=rows, outputs=FULL)
            assert (was, was_full) == (0, 0), dec
            _same(lean, full, (H, W, rows, dec))
    finally:
        r.close()


def test_a_row_tile_is_blocked_and_equals_its_rows_of_the_whole_frame():
    r = _renderer(*_nets("4x128"))
    try:
        pose = bench.sweep_pose(0, 1)
        whole, was_whole = _render(r, 64, 64, pose=pose)
        tile, was_tile = _render(r, 64, 64, pose=pose, rows=(4, 12))
        assert (was_whole, was_tile) == (1, 1)
        for k in LEAN:
            assert torch.equal(tile[k], whole[k][4 * 64:12 * 64]), k
    finally:
        r.close()


def _no_density(sigma):
    return (sigma <= 0) & (sigma >= -FLT_MAX)


def test_the_path_runs_exactly_on_hollow_blocks():
    """Rows [400, 404) of the 800-wide benchmark view: 3 200 rays, 100 packets, one band of 100 blocks.  A NaN in the fine rgb
    head under the test hook that ignores the pack-time guard (colour-skip mode 2): 0 x NaN = NaN wherever a colour layer ran,
    so a ray's rgb is finite if and only if its wave was hollow at every fine sample - with blocks on the wave is the ray's 8x4
    block, with blocks off its run of 32 consecutive rays, both by sigma of the full instantiation.  Depth and acc are the full
    instantiation's either way."""
    sd_c, sd_f = _nets("8x256-0.2")
    sd_f["_rgb_linear.weight"] = sd_f["_rgb_linear.weight"].copy()
    sd_f["_rgb_linear.weight"][1, 3] = np.nan
    r = _renderer(sd_c, sd_f)
    try:
        assert not r.packed_colour_finite(1)
        pose = bench.sweep_pose(0, 1)
        for dec in (0, 1):
            r.debug_set_decomposition(dec)
            full, was_full = _render(r, 800, 800, pose=pose, rows=(400, 404), outputs=FULL)
            assert was_full == 0 and bool(torch.isnan(full["rgb"]).any(dim=1).all())
            none = _no_density(full["raw_fine"][..., 3]).all(dim=1).view(4, 100, 8)            # [row, block, column]: at every fine sample
            by_block = none.all(dim=2).all(dim=0)[None, :, None].expand(4, 100, 8).reshape(-1)   # the ray's 8x4 block
            by_strip = none.view(100, 32).all(dim=1).repeat_interleave(32)                       # its 32 consecutive rays
            shares = float(by_block.float().mean()), float(by_strip.float().mean())
            print("decomposition", dec, "rays of waves hollow at every sample: blocks %.3f, strips %.3f" % shares)
            assert 0.0 < shares[0] < 1.0 and 0.0 < shares[1] < 1.0 and not torch.equal(by_block, by_strip), shares
            r.debug_set_colour_skip(2)
            for blocks, want in ((True, by_block), (False, by_strip)):
                r.debug_set_packet_blocks(blocks)
                hook, was = _render(r, 800, 800, pose=pose, rows=(400, 404))
                assert was == int(blocks)
                assert torch.equal(torch.isfinite(hook["rgb"]).all(dim=1), want), (dec, blocks)
                _same(hook, full, (dec, blocks), keys=("depth", "acc"))
            r.debug_set_packet_blocks(True)
            r.debug_set_colour_skip(1)
    finally:
        r.close()
