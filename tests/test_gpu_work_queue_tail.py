"""The tail path of the work queue on the GPU (include/nwe.h: nwe_debug_set_work_queue, nwe_debug_last_tail; the kernel:
csrc/nwe_mfma_render.h, render_mfma_tail_kernel): under the hybrid plan the surplus workgroups of the queued packets launch render
the sample-split items.  Which workgroup renders a ray changes and nothing about the ray: every comparison is torch.equal on the
raw bits and the flag word, against the same call under the hardware's static dealing (mode 0).

Sizes come from cus = multi_processor_count: g(n) is the grid rule, surplus = g(cus) - cus the workgroups a queued round of packets
starts beyond its items (64 at 256 CUs).  A frame of cus * 128 + k * 32 rays is one round of packets plus k split items and takes
the path exactly if k <= surplus.  Only pinhole frames are lean, so every ray count here is an H x W (x poses) product."""
import pytest
import torch

import nwe_amd
from nwe_amd import _lib, synthetic
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.1, 10.0
LEAN = ("rgb", "depth", "acc")
EVERY = tuple(k for k in _lib.OUTPUT_FIELDS if k not in ("feat_map", "flags"))
NETS = {"4x128": dict(D=4, W=128), "8x256": dict(D=8, W=256), "noview": dict(D=4, W=128, use_view_dirs=False)}


def _pose(yaw=-30.0):
    return O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, yaw, 0.0, 0.0))[0].numpy()


def _kw(H, W):
    fx, fy, cx, cy = O.intrinsics(H, W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR)


def _renderer(net="4x128", ns=7, ni=6):
    r = nwe_amd.Renderer(0)
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
    """As tests/test_gpu_work_queue.py: (items, grid) per launch of a plan over n_rays."""
    full = n_rays // 128 // cus * cus * 128 if plan == 2 else 0
    parts = {0: [(n_rays, 128)], 1: [(n_rays, 32)], 2: [(full, 128), (n_rays - full, 32)]}[plan]
    items = [-(-rays // per) for rays, per in parts] + [0] * (2 - len(parts))
    items = [n if n and queued(n) else 0 for n in items]
    return tuple(items), tuple(_grid(n) if n else 0 for n in items)


def _hw(n):
    """(H, W) with H * W == n, W the divisor of n nearest to its square root; None if n has no divisor that keeps both below 8192."""
    best = None
    for w in range(1, int(n ** 0.5) + 1):
        if n % w == 0 and n // w < 8192:
            best = (w, n // w)
    return best


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def surplus(cus):
    return _grid(cus) - cus


def _qualifying(cus, surplus, rounds=1):
    """Rays of `rounds` full rounds of packets plus as many split items as the packets launch's surplus: the largest frame of
    that many rounds that takes the path."""
    return rounds * cus * 128 + (_grid(rounds * cus) - rounds * cus) * 32


def _ab(r, call, ctx, plan=2, mode=1):
    """call() under mode 0 and under `mode`, bit-equal; returns the queued result's (queue report, stolen, parts under mode 0,
    parts)."""
    r.debug_set_decomposition(plan)
    r.debug_set_work_queue(0)
    want = {k: v.clone() for k, v in call().items()}
    assert r.debug_last_tail() == 0 and r.debug_last_queue()["grid"] == (0, 0), ctx
    parts0 = r.last_launch_parts()
    r.debug_set_work_queue(mode)
    got = call()
    _same(got, want, ctx)
    q, stolen, rest = r.debug_last_queue(), r.debug_last_tail(), r.debug_last_tail_rest()
    # exactly once: what the first launch took and what the second rendered are the plan's split items, and with the surplus
    # covering them the second launch rendered none (a second launch that ignored the counter would report them all)
    assert rest == 0 and (stolen == 0 or stolen == q["items"][1]), (ctx, q, stolen, rest)
    return q, stolen, parts0, r.last_launch_parts()


def test_the_boundary(cus, surplus):
    """One round of packets plus `surplus` split items: the path is taken and every split item is stolen.  One item more: the
    launches are the ones without the path.  The queue report is what _expect_queue says in both."""
    r = _renderer()
    try:
        for extra, stolen in ((0, surplus), (32, 0)):
            n = cus * 128 + surplus * 32 + extra
            H, W = _hw(n)
            q, got, _, _ = _ab(r, lambda: r.render(_pose(), H, W, outputs=LEAN, **_kw(H, W)), (n, H, W))
            print("rays", n, "frame", (H, W), "queue", q, "stolen", got)
            assert got == stolen, (n, q)
            items, grid = _expect_queue(2, n, cus, lambda m: True)
            assert (q["items"], q["grid"], q["taken"]) == (items, grid, grid) and q["side_stream"], (n, q)
            assert r.debug_last_plan() == 2
    finally:
        r.close()


def test_a_ragged_last_packet(cus, surplus):
    """The last split item 5 rays wide (one pose) or 6 (two poses, whose ray count is even): the ray count is no multiple of
    32.  k split items with k the largest count up to the surplus whose ray count is an H x W product."""
    r = _renderer()
    try:
        for poses, width in (([_pose()], 5), ([_pose(), _pose(-75.0)], 6)):
            k, hw = next((k, _hw((cus * 128 + (k - 1) * 32 + width) // len(poses))) for k in range(surplus, 0, -1)
                         if (cus * 128 + (k - 1) * 32 + width) % len(poses) == 0 and _hw((cus * 128 + (k - 1) * 32 + width) // len(poses)))
            H, W = hw
            n = len(poses) * H * W
            assert n == cus * 128 + (k - 1) * 32 + width and n % 32
            q, stolen, _, _ = _ab(r, lambda: r.render(poses, H, W, outputs=LEAN, **_kw(H, W)), (len(poses), H, W))
            print("poses", len(poses), "frame", (H, W), "split items", k, "queue", q, "stolen", stolen)
            assert stolen == k == q["items"][1], (q, stolen)
            assert q["taken"] == q["grid"] and q["side_stream"]
    finally:
        r.close()


def test_not_lean(cus, surplus):
    """render_rays with every output on the qualifying ray count: the full kernels have no tail variant."""
    r = _renderer()
    try:
        H, W = _hw(_qualifying(cus, surplus))
        rays = r.create_rays(_pose(), H, W, **_kw(H, W))
        q, stolen, _, _ = _ab(r, lambda: r.render_rays(rays, outputs=EVERY), "every output")
        assert stolen == 0 and any(q["grid"]) and q["taken"] == q["grid"]
        q, stolen, _, _ = _ab(r, lambda: r.render_rays(rays, outputs=LEAN), "precomputed rays, lean outputs")
        assert stolen == 0 and any(q["grid"])             # precomputed rays are not a lean call either
    finally:
        r.close()


@pytest.mark.parametrize("net, ns, ni, precs", [("8x256", 64, 128, ("f16x3", "f16x1")), ("noview", 7, 6, ("f16x3",))])
def test_shapes_and_precisions(net, ns, ni, precs, cus, surplus):
    r = _renderer(net, ns, ni)
    try:
        H, W = _hw(_qualifying(cus, surplus))
        for prec in precs:
            q, stolen, _, _ = _ab(r, lambda: r.render(_pose(), H, W, precision=prec, outputs=LEAN, **_kw(H, W)), (net, prec))
            assert stolen == q["items"][1] == surplus, (net, prec, q, stolen)
    finally:
        r.close()


def test_default_mode(cus):
    """Five full rounds plus g(5 cus) - 5 cus split items: more than cus workgroups in each launch, so both are queued under the
    default mode, and the automatic plan is the hybrid one."""
    r = _renderer()
    try:
        n = _qualifying(cus, None, rounds=5)
        items1 = _grid(5 * cus) - 5 * cus
        assert items1 > cus
        H, W = _hw(n)
        q, stolen, parts0, parts = _ab(r, lambda: r.render(_pose(), H, W, outputs=LEAN, **_kw(H, W)), "default mode", plan=-1, mode=-1)
        assert r.debug_last_plan() == 2
        items, grid = _expect_queue(2, n, cus, lambda m: m > cus)
        assert all(items) and (q["items"], q["grid"], q["taken"]) == (items, grid, grid) and q["side_stream"], q
        assert stolen == items1 == items[1]
    finally:
        r.close()


def test_parts(cus, surplus):
    """Two positive parts with the rays of the plan's two launches, adding up to the kernel time."""
    r = _renderer()
    try:
        H, W = _hw(_qualifying(cus, surplus))
        q, stolen, parts0, parts = _ab(r, lambda: r.render(_pose(), H, W, outputs=LEAN, **_kw(H, W)), "parts")
        ms = r.last_kernel_ms()
        print("parts", parts, "static", parts0, "kernel ms", ms)
        assert stolen == surplus
        assert len(parts) == 2 and all(p[0] > 0 for p in parts) and [p[1] for p in parts] == [p[1] for p in parts0] == [cus * 128, surplus * 32]
        assert abs(sum(p[0] for p in parts) - ms) <= 1e-4 * ms + 2e-5, (parts, ms)
    finally:
        r.close()


def test_long_lived_context(monkeypatch, cus, surplus):
    """Six qualifying renders on six streams equal the serial renders, twice: the third counter is zeroed per call and per slot.
    The mode toggled between launches, and a context created under NWE_WORK_QUEUE_TAIL=0 beside one without it.  A refused launch
    leaves nwe_debug_last_tail, the queue report and the timing calls describing the last good launch."""
    monkeypatch.setenv("NWE_WORK_QUEUE_TAIL", "0")
    off = _renderer()
    monkeypatch.delenv("NWE_WORK_QUEUE_TAIL")
    r = _renderer()
    assert r.debug_get_work_queue_tail() is True and off.debug_get_work_queue_tail() is False   # fixed at creation: no run-time switch
    yaws = (0.0, -25.0, -50.0, -75.0, -100.0, -125.0)
    H, W = _hw(_qualifying(cus, surplus))
    kw = dict(outputs=LEAN, **_kw(H, W))
    try:
        for x in (r, off):
            x.debug_set_decomposition(2)
        r.debug_set_work_queue(0)
        want = [{k: v.clone() for k, v in r.render(_pose(y), H, W, **kw).items()} for y in yaws]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in yaws]
        r.debug_set_work_queue(1)
        for _ in range(2):
            got = []
            for y, st in zip(yaws, streams):
                with torch.cuda.stream(st):
                    got.append(r.render(_pose(y), H, W, **kw))
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(got, want)):
                _same(a, b, ("six streams", i))
            assert r.debug_last_tail() == surplus and r.debug_last_tail_rest() == 0
        # the mode and the switch toggled between launches
        off.debug_set_work_queue(1)
        for i, mode in enumerate((1, 0, -1, 1, 0, 1)):
            r.debug_set_work_queue(mode)
            _same(r.render(_pose(yaws[i]), H, W, **kw), want[i], ("toggle", i, mode))
            assert r.debug_last_tail() == (surplus if mode == 1 else 0), (i, mode)    # mode -1: a round of cus packets is not queued
            _same(off.render(_pose(yaws[i]), H, W, **kw), want[i], ("switched off", i))
            q = off.debug_last_queue()
            assert off.debug_last_tail() == 0 and off.debug_last_tail_rest() == 0 and q["items"] == (cus, surplus) and q["side_stream"], (i, q)
            assert q["taken"] == q["grid"] == (_grid(cus), _grid(surplus)), (i, q)
            if mode == 1:
                assert r.debug_last_queue() == q, (i, r.debug_last_queue(), q)   # the path changes nothing of the report
        # a refused launch: coarse and fine networks of different shapes under an MFMA precision
        r.debug_set_work_queue(1)
        r.render(_pose(), H, W, **kw)
        state = (r.last_kernel_ms(), r.last_launch_parts(), r.debug_last_queue(), r.debug_last_tail(), r.debug_last_tail_rest())
        assert state[3] == surplus and state[4] == 0 and len(state[1]) == 2
        r.set_network(0, synthetic.make_state_dict(1000, **NETS["8x256"]))
        for _ in range(5):                                    # more refusals than the ring has slots
            with pytest.raises(NotImplementedError, match="same shape"):
                r.render(_pose(), H, W, precision="f16x3", **kw)
            assert (r.last_kernel_ms(), r.last_launch_parts(), r.debug_last_queue(), r.debug_last_tail(), r.debug_last_tail_rest()) == state
    finally:
        r.close(); off.close()


def test_modes_that_stay_static(cus, surplus):
    """Early termination, the shared coarse pass (k = 2) and separate passes on a qualifying ray count keep their launches."""
    r = _renderer()
    H, W = _hw(_qualifying(cus, surplus))
    modes = {"early termination": (lambda on: r.set_early_termination(1e-2 if on else 0.0)),
             "shared coarse": (lambda on: r.set_shared_coarse(2 if on else 1)),
             "separate passes": (lambda on: r.set_separate_passes(on))}
    try:
        for name, switch in modes.items():
            switch(True)
            r.debug_set_decomposition(2)
            res = {}
            for mode in (0, 1):
                r.debug_set_work_queue(mode)
                res[mode] = {k: v.clone() for k, v in r.render(_pose(), H, W, outputs=LEAN, **_kw(H, W)).items()}
                assert r.debug_last_tail() == 0 and r.debug_last_queue()["grid"] == (0, 0), (name, mode)
            _same(res[1], res[0], name)
            switch(False)
        r.render(_pose(), H, W, outputs=LEAN, **_kw(H, W))    # and the plain call behind them takes the path again
        assert r.debug_last_tail() == surplus
    finally:
        r.close()
