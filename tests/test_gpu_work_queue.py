"""The work queue on the GPU (include/nwe.h: nwe_debug_set_work_queue; the kernel's part: csrc/nwe_mfma_render.h).  A queued launch
changes which workgroup renders a ray and nothing about the ray: every comparison here is torch.equal on the raw bits, against
the same call under the hardware's static dealing (mode 0)."""
import pytest
import torch

import nwe_amd
from nwe_amd import _lib, synthetic
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.1, 10.0
LEAN = ("rgb", "depth", "acc")
EVERY = tuple(k for k in _lib.OUTPUT_FIELDS if k not in ("feat_map", "flags"))   # feat_map: the f32 kernel's only
NETS = {"4x128": dict(D=4, W=128), "8x256": dict(D=8, W=256), "noview": dict(D=4, W=128, use_view_dirs=False)}


def _pose(yaw=-30.0):
    return O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, yaw, 0.0, 0.0))[0].numpy()


def _kw(H, W):
    fx, fy, cx, cy = O.intrinsics(H, W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR)


def _renderer(net="8x256", ns=64, ni=128, cls=nwe_amd.Renderer, arg=0):
    r = cls(arg)
    r.set_network(0, synthetic.make_state_dict(1000, **NETS[net]))
    r.set_network(1, synthetic.make_state_dict(1001, **NETS[net]))
    r.set_sampling(ns, ni)
    return r


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want, ctx):
    assert set(got) == set(want)
    for k in want:                                       # the flag word included
        assert torch.equal(_bits(got[k]), _bits(want[k])), (ctx, k)


def _grid(n):
    return (n + (n + 3) // 4 + 7) // 8 * 8


def _expect_queue(plan, n_rays, cus, queued):
    """(items, grid) per launch of a plan over n_rays; queued(workgroups) says whether a launch of that size is dealt from a queue."""
    full = n_rays // 128 // cus * cus * 128 if plan == 2 else 0
    parts = {0: [(n_rays, 128)], 1: [(n_rays, 32)], 2: [(full, 128), (n_rays - full, 32)]}[plan]
    items = [-(-rays // per) for rays, per in parts] + [0] * (2 - len(parts))
    items = [n if n and queued(n) else 0 for n in items]
    return tuple(items), tuple(_grid(n) if n else 0 for n in items)


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("ns, ni", [(64, 128), (7, 6)])
@pytest.mark.parametrize("net", sorted(NETS))
def test_forced_queue_on_frames_far_smaller_than_the_device(net, ns, ni, cus):
    """Mode 1 against mode 0 where most of the over-provisioned grid takes the exit path: 7x19 with two poses (266 rays: two full
    groups and a ragged packet) and 12x64, the three forced plans, both MFMA precisions, lean frames and render_rays with every
    output.  Outputs and flag word equal; items = ceil(rays / rays per workgroup), grid by the rule, every workgroup took a ticket."""
    r = _renderer(net, ns, ni)
    try:
        for H, W, poses in ((7, 19, [_pose(), _pose(-75.0)]), (12, 64, [_pose()])):
            n_rays = len(poses) * H * W
            rays = r.create_rays(poses, H, W, use_view_dirs=net != "noview", **_kw(H, W))
            calls = {"lean frame": lambda prec: r.render(poses, H, W, precision=prec, outputs=LEAN, **_kw(H, W)),
                     "render_rays, every output": lambda prec: r.render_rays(rays, precision=prec, outputs=EVERY)}
            for plan in (0, 1, 2):
                r.debug_set_decomposition(plan)
                for prec in ("f16x3", "f16x1"):
                    for what, call in calls.items():
                        ctx = (net, ns, ni, H, W, plan, prec, what)
                        r.debug_set_work_queue(0)
                        want = call(prec)
                        q0 = r.debug_last_queue()
                        assert q0 == {"items": (0, 0), "grid": (0, 0), "taken": (0, 0), "side_stream": False}, ctx
                        r.debug_set_work_queue(1)
                        got = call(prec)
                        _same(got, want, ctx)
                        q = r.debug_last_queue()
                        items, grid = _expect_queue(plan, n_rays, cus, lambda n: True)
                        assert (q["items"], q["grid"], q["taken"]) == (items, grid, grid), (ctx, q)
                        assert r.debug_last_plan() == plan and q["side_stream"] == (plan == 2), (ctx, q)
    finally:
        r.close()


def test_more_workgroups_than_cus(cus):
    """200x300 at 4x128 and 7+6 samples (60000 rays: one round of packets on 256 CUs plus 27232 rays split): tickets are taken by
    workgroups that had to wait for a CU.  The default mode against mode 0 under plans 0, 1 and 2: same bits, same plan, same
    rays per part; two positive parts that sum to the kernel time; under plan 2 the second launch ran on the renderer's stream."""
    r = _renderer("4x128", 7, 6)
    H, W = 200, 300
    try:
        assert r.debug_get_work_queue() in (-1, 0, 1)
        for plan in (0, 1, 2):
            r.debug_set_decomposition(plan)
            r.debug_set_work_queue(0)
            want = r.render(_pose(), H, W, outputs=LEAN, **_kw(H, W))
            parts0 = r.last_launch_parts()
            assert r.debug_last_queue()["grid"] == (0, 0)
            r.debug_set_work_queue(-1)
            got = r.render(_pose(), H, W, outputs=LEAN, **_kw(H, W))
            _same(got, want, plan)
            parts, ms, q = r.last_launch_parts(), r.last_kernel_ms(), r.debug_last_queue()
            print("plan", plan, "parts", parts, "static", parts0, "queue", q)
            assert r.debug_last_plan() == plan and [p[1] for p in parts] == [p[1] for p in parts0]
            assert len(parts) == (2 if plan == 2 else 1) and all(p[0] > 0 for p in parts)
            assert abs(sum(p[0] for p in parts) - ms) <= 1e-4 * ms + 2e-5, (parts, ms)   # float32 sums of two 10 ns-step event times
            items, grid = _expect_queue(plan, H * W, cus, lambda n: n > cus)
            assert (q["items"], q["grid"], q["taken"]) == (items, grid, grid), (plan, q)
            assert q["side_stream"] == (plan == 2 and any(grid))
            if plan == 2:
                assert sum(p[1] for p in parts) == H * W and parts[0][1] == H * W // 128 // cus * cus * 128
    finally:
        r.close()


def test_long_lived_context(cus):
    """Six renders on six streams with mode 1 equal the serial renders, twice, so that every slot, its counters and its stream
    are reused; the mode toggled between launches; 96x128 after 200x300; a refused launch leaves nwe_debug_last_queue and the
    timing calls describing the last good launch."""
    r = _renderer()
    yaws = (0.0, -25.0, -50.0, -75.0, -100.0, -125.0)
    kw = dict(outputs=LEAN, **_kw(96, 128))
    try:
        r.debug_set_work_queue(0)
        r.debug_set_decomposition(2)
        want = [{k: v.clone() for k, v in r.render(_pose(y), 96, 128, **kw).items()} for y in yaws]
        big = r.render(_pose(), 200, 300, outputs=LEAN, **_kw(200, 300))
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in yaws]
        r.debug_set_work_queue(1)
        for _ in range(2):
            got = []
            for y, st in zip(yaws, streams):
                with torch.cuda.stream(st):
                    got.append(r.render(_pose(y), 96, 128, **kw))
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(got, want)):
                _same(a, b, ("six streams", i))
            q = r.debug_last_queue()
            assert q["items"] == (0, 96 * 128 // 32) and q["taken"] == q["grid"] == (0, _grid(96 * 128 // 32)) and q["side_stream"]
        # the mode toggled between launches, the large frame in front of the small one
        for i, mode in enumerate((1, 0, -1, 1, 0, 1)):
            r.debug_set_work_queue(mode)
            _same(r.render(_pose(), 200, 300, outputs=LEAN, **_kw(200, 300)), big, ("toggle, 200x300", i, mode))
            assert any(r.debug_last_queue()["grid"]) == (mode == 1 or (mode == -1 and 27232 // 32 > cus))
            _same(r.render(_pose(yaws[i]), 96, 128, **kw), want[i], ("toggle, 96x128", i, mode))
            assert any(r.debug_last_queue()["grid"]) == (mode == 1 or (mode == -1 and 96 * 128 // 32 > cus))
        # a refused launch: coarse and fine networks of different shapes under an MFMA precision
        r.debug_set_work_queue(1)
        r.render(_pose(), 200, 300, outputs=LEAN, **_kw(200, 300))
        ms, parts, q = r.last_kernel_ms(), r.last_launch_parts(), r.debug_last_queue()
        assert len(parts) == 2 and any(q["grid"]) and q["taken"] == q["grid"]
        r.set_network(0, synthetic.make_state_dict(1000, **NETS["4x128"]))
        for _ in range(5):                                    # more refusals than the ring has slots
            with pytest.raises(NotImplementedError, match="same shape"):
                r.render(_pose(), 7, 19, precision="f16x3", outputs=LEAN, **_kw(7, 19))
            assert (r.last_kernel_ms(), r.last_launch_parts(), r.debug_last_queue()) == (ms, parts, q)
    finally:
        r.close()


def test_backfill_switched_off_by_the_environment(monkeypatch, cus):
    """NWE_WORK_QUEUE_BACKFILL=0: the same queued launches, the second on the caller's stream; same bits.  And a frame smaller than
    the device under the default mode is not queued at all."""
    monkeypatch.setenv("NWE_WORK_QUEUE_BACKFILL", "0")
    r = _renderer("4x128", 7, 6)
    monkeypatch.delenv("NWE_WORK_QUEUE_BACKFILL")
    f = _renderer("4x128", 7, 6)
    try:
        for x in (r, f):
            x.debug_set_decomposition(2)
        got, want = r.render(_pose(), 200, 300, outputs=LEAN, **_kw(200, 300)), f.render(_pose(), 200, 300, outputs=LEAN, **_kw(200, 300))
        _same(got, want, "no backfill")
        q, qf = r.debug_last_queue(), f.debug_last_queue()
        assert q["side_stream"] is False and qf["side_stream"] is True
        assert {k: q[k] for k in ("items", "grid", "taken")} == {k: qf[k] for k in ("items", "grid", "taken")} and any(q["grid"])
        parts, ms = r.last_launch_parts(), r.last_kernel_ms()
        assert len(parts) == 2 and all(p[0] > 0 for p in parts) and abs(sum(p[0] for p in parts) - ms) <= 1e-4 * ms + 2e-5
        f.debug_set_decomposition(-1)
        f.render(_pose(), 12, 64, outputs=LEAN, **_kw(12, 64))          # 768 rays: fewer workgroups than CUs under every plan
        assert f.debug_last_queue() == {"items": (0, 0), "grid": (0, 0), "taken": (0, 0), "side_stream": False}
    finally:
        r.close(); f.close()


def test_modes_that_stay_static():
    """Early termination, the shared coarse pass (k = 2) and separate passes keep their launches: with mode 1 set they equal the
    same calls with mode 0 and report no queue."""
    r = _renderer()
    H, W = 12, 64
    none = {"items": (0, 0), "grid": (0, 0), "taken": (0, 0), "side_stream": False}
    modes = {"early termination": (lambda on: r.set_early_termination(1e-2 if on else 0.0)),
             "shared coarse": (lambda on: r.set_shared_coarse(2 if on else 1)),
             "separate passes": (lambda on: r.set_separate_passes(on))}
    try:
        for name, switch in modes.items():
            switch(True)
            for plan in (-1, 0, 1, 2):
                r.debug_set_decomposition(plan)
                res = {}
                for mode in (0, 1):
                    r.debug_set_work_queue(mode)
                    res[mode] = r.render(_pose(), H, W, outputs=LEAN, **_kw(H, W))
                    assert r.debug_last_queue() == none, (name, plan, mode)
                _same(res[1], res[0], (name, plan))
            switch(False)
        # and the plain call behind them is queued again
        r.debug_set_decomposition(-1)
        r.render(_pose(), H, W, outputs=LEAN, **_kw(H, W))
        assert any(r.debug_last_queue()["grid"])
        r.render(_pose(), H, W, precision="f32", outputs=LEAN, **_kw(H, W))
        assert r.debug_last_queue() == none                   # the f32 kernel has no queue
    finally:
        r.close()


def test_row_tiles_pose_batches_and_tiled_renderer():
    """With mode 1 row tiles, pose batches and TiledRenderer([0, 0, 0]) are bit-identical to the whole frame."""
    H, W = 30, 40
    r = _renderer()
    t = _renderer(cls=nwe_amd.TiledRenderer, arg=[0, 0, 0])
    poses = [_pose(), _pose(-80.0)]
    try:
        r.debug_set_work_queue(0)
        whole = [r.render(p, H, W, outputs=LEAN, **_kw(H, W)) for p in poses]
        r.debug_set_work_queue(1)
        t.debug_set_work_queue(1)
        for plan in (-1, 0, 2):
            r.debug_set_decomposition(plan)
            batch = r.render(poses, H, W, outputs=LEAN, **_kw(H, W))
            for k in LEAN:
                assert torch.equal(_bits(batch[k]), _bits(torch.cat([w[k] for w in whole]))), (plan, "pose batch", k)
            tiles = [r.render(poses[0], H, W, rows=rows, outputs=LEAN, **_kw(H, W)) for rows in ((0, 7), (7, 8), (8, 30))]
            for k in LEAN:
                assert torch.equal(_bits(torch.cat([x[k] for x in tiles])), _bits(whole[0][k])), (plan, "row tiles", k)
            assert any(r.debug_last_queue()["grid"])
        tiled = t.render(poses[0], H, W, outputs=LEAN, **_kw(H, W))
        torch.cuda.synchronize()
        assert t.last_tiled
        for k in LEAN:
            assert torch.equal(_bits(tiled[k]), _bits(whole[0][k])), ("TiledRenderer", k)
        assert all(any(p.debug_last_queue()["grid"]) for p in t.parts)
    finally:
        r.close(); t.close()
