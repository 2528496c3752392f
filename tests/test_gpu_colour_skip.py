"""The hollow path of the lean MFMA kernels (csrc/nwe_mfma_eval.h: mlp_eval, CSKIP; include/nwe.h: nwe_debug_set_colour_skip).

In the pass that produces the outputs, a wave whose 32 rays all have sigma_raw <= 0 at a sample leaves out the colour layers of
that evaluation: the sample weighs 0 on every ray.  The unit is (packet of 32 consecutive rays, sample) in both work
decompositions.  The small frames of the other GPU tests never take the path - their 32 consecutive rays span the whole field of
view - so the rays here are coherent: a few rows of the 800-wide benchmark frame under the benchmark's pose.  This file takes the
path in the plain and tail kernels at 8x256 and 4x128 (tests/test_gpu_packet_blocks.py likewise); the terminating, occupancy and
sharing kernels, and the plain kernels of 4x256 and 8x128, take it in tests/test_gpu_hollow_variants.py.

Predictions come from the kernel's own sigma: raw_fine (raw_coarse without importance sampling) of the FULL instantiation of
the same call, which never takes the path.  Every comparison is torch.equal."""
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
FLAGS_KEPT = 0x7                     # fine rgb / depth / acc: the bits a lean frame and a full frame share whatever else is asked for
FLT_MAX = float(np.finfo(np.float32).max)
SAMPLINGS = ((64, 128), (37, 17), (37, 0))


def _nets(name):
    """(coarse, fine).  8x256: the benchmark's networks.  4x128 has no packet without density on these rows as it is (the oracle:
    0.00), so the density bias of its fine network is lowered."""
    D, W, shift = {"8x256": (8, 256, 0.0), "4x128": (4, 128, 0.3), "8x256-0.2": (8, 256, 0.2)}[name]
    sd_c, sd_f = synthetic.make_state_dict(1000, D, W), synthetic.make_state_dict(1001, D, W)
    sd_f["_alpha_linear.bias"] = (sd_f["_alpha_linear.bias"] - np.float32(shift)).astype(np.float32)
    return sd_c, sd_f


def _renderer(sd_c, sd_f):
    r = nwe_amd.Renderer(0)
    r.set_network(0, sd_c)
    r.set_network(1, sd_f)
    return r


def _rows(r, rows, precision="f16x3", outputs=LEAN, size=800, pose=None):
    fx, fy, cx, cy = O.intrinsics(size, size)
    pose = bench.sweep_pose(0, 1) if pose is None else pose
    return r.render(pose, size, size, fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR, rows=rows, precision=precision, outputs=outputs)


def _full(r, rows, precision="f16x3", **kw):
    """The full instantiation of the call, and its sigma [rays, samples] in the pass that produces the outputs."""
    raw = "raw_fine" if r.n_importance > 0 else "raw_coarse"
    out = _rows(r, rows, precision, LEAN + (raw,), **kw)
    return out, out[raw][..., 3]


def _hollow(sigma):
    """[packets, samples]: no ray of the packet has density at the sample.  The lanes of a ragged last packet compute the call's
    last ray along (csrc/nwe_mfma_render_item.h), so they add nothing to the packet's vote."""
    R, S = sigma.shape
    none = (sigma <= 0) & (sigma >= -FLT_MAX)
    pad = (-R) % 32
    if pad:
        none = torch.cat([none, none[-1:].expand(pad, S)])
    return none.view(-1, 32, S).all(dim=1)


def _same(a, b, ctx, keys=LEAN):
    for k in keys:
        assert torch.equal(a[k], b[k]), (ctx, k)
    fa, fb = int(a["flags"].item()), int(b["flags"].item())
    assert fa & FLAGS_KEPT == fb & FLAGS_KEPT, (ctx, hex(fa), hex(fb))


@pytest.mark.parametrize("net", ["8x256", "4x128"])
def test_lean_equals_full_and_mode_1_equals_mode_0(net):
    """Rows [400, 402) = 1600 rays = 50 packets, 64 + 128 / 37 + 17 / 37 + 0 samples, decompositions 0 / 1 / 2, both MFMA
    precisions: the lean frame with the path on is the full frame and the lean frame with the path off, bit for bit, and between
    a tenth and nine tenths of the (packet, sample) pairs of the call are hollow by the full frame's own sigma.  Without
    importance sampling the single pass produces the outputs, with network 0: there the fine network sits in that slot, so that
    the call has the same density as the others."""
    sd_c, sd_f = _nets(net)
    r = _renderer(sd_c, sd_f)
    try:
        for ns, ni in SAMPLINGS:
            r.set_network(0, sd_c if ni > 0 else sd_f)
            r.set_sampling(ns, ni)
            for precision in ("f16x3", "f16x1"):
                r.debug_set_decomposition(0)
                full, sigma = _full(r, (400, 402), precision)
                share = float(_hollow(sigma).float().mean())
                print(net, ns, ni, precision, "hollow share %.3f" % share)
                assert 0.1 <= share <= 0.9, (net, ns, ni, precision, share)
                for mode in (0, 1, 2):
                    r.debug_set_decomposition(mode)
                    ctx = (net, ns, ni, precision, mode)
                    r.debug_set_colour_skip(1)
                    on = _rows(r, (400, 402), precision)
                    r.debug_set_colour_skip(0)
                    off = _rows(r, (400, 402), precision)
                    _same(on, full, ctx)
                    _same(on, off, ctx)
    finally:
        r.close()


@pytest.mark.parametrize("rows,size", [((400, 402), 800), ((395, 396), 790)], ids=["50-packets", "24-packets-and-22-rays"])
def test_the_path_runs_exactly_where_predicted(rows, size):
    """A NaN in the fine rgb head and the test hook that ignores the pack-time guard (mode 2): a ray's rgb is finite if and only if
    its packet is hollow at every sample of the fine pass - 0 x NaN = NaN wherever the colour layers ran.  Depth and acc are the
    full frame's.  Under mode 1 the pack-time guard keeps every evaluation on the full path: every ray's rgb is NaN."""
    sd_c, sd_f = _nets("8x256-0.2")
    sd_f["_rgb_linear.weight"] = sd_f["_rgb_linear.weight"].copy()
    sd_f["_rgb_linear.weight"][1, 3] = np.nan
    r = _renderer(sd_c, sd_f)
    try:
        assert not r.packed_colour_finite(1) and r.packed_colour_finite(0)
        for ns, ni in ((64, 128), (37, 17)):
            r.set_sampling(ns, ni)
            for mode in (0, 1):
                r.debug_set_decomposition(mode)
                full, sigma = _full(r, rows, size=size)
                assert torch.isnan(full["rgb"]).any(dim=1).all()
                hollow_ray = _hollow(sigma).all(dim=1).repeat_interleave(32)[:sigma.shape[0]]
                share = float(hollow_ray.float().mean())
                print(rows, ns, ni, mode, "rays of packets hollow at every sample: %.3f" % share)
                assert 0.2 <= share <= 0.8, (rows, ns, ni, mode, share)
                r.debug_set_colour_skip(2)
                hook = _rows(r, rows, size=size)
                assert torch.equal(torch.isfinite(hook["rgb"]).all(dim=1), hollow_ray), (rows, ns, ni, mode)
                _same(hook, full, (rows, ns, ni, mode), keys=("depth", "acc"))
                r.debug_set_colour_skip(1)
                guarded = _rows(r, rows, size=size)
                assert torch.isnan(guarded["rgb"]).any(dim=1).all(), (rows, ns, ni, mode)
                _same(guarded, full, (rows, ns, ni, mode), keys=("depth", "acc"))
    finally:
        r.close()


def test_ragged_packets():
    """Rows [395, 396) of a 790 x 790 frame: 24 packets and 22 rays.  Lean with the path on = full = lean with the path off."""
    r = _renderer(*_nets("8x256"))
    try:
        r.set_sampling(37, 17)
        for mode in (0, 1):
            r.debug_set_decomposition(mode)
            full, sigma = _full(r, (395, 396), size=790)
            assert sigma.shape[0] == 24 * 32 + 22
            hollow = _hollow(sigma)
            assert 0.1 <= float(hollow.float().mean()) <= 0.9, mode
            r.debug_set_colour_skip(1)
            on = _rows(r, (395, 396), size=790)
            r.debug_set_colour_skip(0)
            off = _rows(r, (395, 396), size=790)
            _same(on, full, mode)
            _same(on, off, mode)
    finally:
        r.close()


def test_zero_rotation_never_takes_the_path():
    """A zero rotation: d = 0, the view direction 0 / 0, gamma(d) NaN, while every sample point - the origin - and so sigma stay
    finite.  With the density bias lowered far enough no sample has density, so every (packet, sample) pair would be hollow;
    the per-ray guard keeps the waves on the full path, and the lean frame is the full frame, NaN colour included."""
    sd_c, sd_f = _nets("4x128")
    sd_f["_alpha_linear.bias"] = (sd_f["_alpha_linear.bias"] - np.float32(50.0)).astype(np.float32)
    pose = bench.sweep_pose(0, 1).copy()
    pose[:3, :3] = 0.0
    r = _renderer(sd_c, sd_f)
    try:
        r.set_sampling(37, 17)
        for mode in (0, 1):
            r.debug_set_decomposition(mode)
            full, sigma = _full(r, (400, 402), pose=pose)
            assert bool(_hollow(sigma).all()) and bool(torch.isnan(full["rgb"]).all())
            for skip in (1, 2):
                r.debug_set_colour_skip(skip)
                lean = _rows(r, (400, 402), pose=pose)
                for k in LEAN:
                    assert torch.equal(torch.isnan(lean[k]), torch.isnan(full[k])), (mode, skip, k)
                    assert torch.equal(torch.nan_to_num(lean[k], nan=7.0), torch.nan_to_num(full[k], nan=7.0)), (mode, skip, k)
    finally:
        r.close()


def _grid(n):
    return (n + (n + 3) // 4 + 7) // 8 * 8


def _hw(n):
    """(H, W) with H * W == n, W the divisor of n nearest to its square root (tests/test_gpu_work_queue_tail.py)."""
    best = None
    for w in range(1, int(n ** 0.5) + 1):
        if n % w == 0 and n // w < 8192:
            best = (w, n // w)
    return best


def test_hybrid_plan_and_tail_path():
    """60 000 coherent rays (rows [360, 435)) at 8x256, 64 + 128 under the launcher's own plan, and the smallest call that takes
    the tail path - one round of packets and one sample-split item, every launch queued: the path on = the path off, bit for
    bit, under the same plan and with the same split items rendered in the packets launch's tail."""
    r = _renderer(*_nets("8x256"))
    try:
        r.set_sampling(64, 128)
        got = {}
        for skip in (0, 1):
            r.debug_set_colour_skip(skip)
            got[skip] = _rows(r, (360, 435))
            got[skip]["plan"] = r.debug_last_plan()
        assert got[0]["plan"] == got[1]["plan"]
        _same(got[1], got[0], "60000 rays")
        assert float(torch.isfinite(got[1]["rgb"]).float().mean()) == 1.0
    finally:
        r.close()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * 128 + 32
    assert _grid(cus) - cus >= 1
    H, W = _hw(n)
    fx, fy, cx, cy = O.intrinsics(H, W)
    r = _renderer(*_nets("4x128"))
    try:
        r.set_sampling(7, 6)
        r.debug_set_decomposition(2)
        r.debug_set_work_queue(1)
        got = {}
        for skip in (0, 1):
            r.debug_set_colour_skip(skip)
            got[skip] = r.render(bench.sweep_pose(0, 1), H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR, outputs=LEAN)
            got[skip]["plan"], got[skip]["tail"] = r.debug_last_plan(), r.debug_last_tail()
        assert got[0]["plan"] == got[1]["plan"] == 2 and got[0]["tail"] == got[1]["tail"] == 1, (got[0]["plan"], got[0]["tail"], got[1]["tail"])
        _same(got[1], got[0], ("tail", n, H, W))
    finally:
        r.close()


def test_the_switch():
    r = nwe_amd.Renderer(0)
    try:
        assert r.debug_get_colour_skip() == 1
        for mode in (0, 2, 1):
            r.debug_set_colour_skip(mode)
            assert r.debug_get_colour_skip() == mode
        for bad in (-1, 3):
            with pytest.raises(Exception):
                r.debug_set_colour_skip(bad)
        assert r.debug_get_colour_skip() == 1
    finally:
        r.close()
