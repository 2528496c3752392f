"""The launches of a real call are the ones the planner names (include/nwe.h: nwe_debug_plan): for every mode of a render call,
what the call reports afterwards - plan, queue, tail, launch parts, coarse launch, evaluations - equals what nwe_debug_plan says
for the same call at the device's CU count.  The planner itself is tested without a GPU, at every CU count, in
tests/test_plan_host.py; the pixels of every mode in the suites of the modes.  Here: the smallest shape that can still go wrong
(4 x 128 networks, 8 + 8 samples) and the ray counts at which a plan changes."""
import ctypes as C

import pytest
import torch

import nwe_amd
from nwe_amd import _lib, synthetic
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.1, 10.0
LEAN = ("rgb", "depth", "acc")


def _grid(n):
    return (n + (n + 3) // 4 + 7) // 8 * 8


def _hw(n):
    """(H, W) with H * W == n, W the divisor of n nearest to its square root (as tests/test_gpu_work_queue_tail.py)."""
    best = None
    for w in range(1, int(n ** 0.5) + 1):
        if n % w == 0 and n // w < 8192:
            best = (w, n // w)
    return best


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def renderer():
    r = nwe_amd.Renderer(0)
    for which in (0, 1):
        r.set_network(which, synthetic.make_state_dict(1000 + which, D=4, W=128))
    r.set_sampling(8, 8)
    yield r
    r.close()


@pytest.fixture(scope="module")
def pose():
    return O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()


def _counts(cus, long=False):
    """A single split item; one round of packets; a round and five split items (tail path); one item past the tail boundary;
    two rounds and three items."""
    counts = [32, cus * 128, cus * 128 + 160, cus * 128 + (_grid(cus) - cus + 1) * 32]
    return counts + [2 * cus * 128 + 96] if long else counts


def _reports(r):
    """What the last call reports about its launches, in the planner's terms."""
    lib = _lib.load()
    q = r.debug_last_queue()
    ms2, rays2 = (C.c_float * 2)(), (C.c_int64 * 2)()
    assert lib.nwe_last_launch_parts(r._ctx, ms2, rays2) == _lib.NWE_OK
    coarse = r.last_coarse_launch()
    return dict(plan=r.debug_last_plan(), items=q["items"], grid=q["grid"], side=q["side_stream"],
                tail=r.debug_last_tail() + r.debug_last_tail_rest(), rays=tuple(rays2), coarse_rays=coarse[1] if coarse else 0,
                evals_full=r.last_ray_evaluations()[1])


def _planned(r, cus, outputs, camera=None, n_rays=-1, hooks=0):
    n_poses, H, W = camera if camera else (0, 0, 0)
    report = _lib.PlanReport()
    out = _lib.Outputs(**{k: 1 for k in outputs})
    rc = _lib.load().nwe_debug_plan(r._ctx, n_poses, H, W, 0, H, n_rays, C.byref(out), hooks, _lib.PREC_F16X3, cus, C.byref(report))
    assert rc == _lib.NWE_OK, _lib.load().nwe_last_error(r._ctx)
    m = report.main
    total = m.rays[0] + m.rays[1]
    return dict(plan=m.plan, items=tuple(m.items[i] if m.grid[i] else 0 for i in (0, 1)), grid=tuple(m.grid), side=m.fork != 0,
                tail=m.tail_items, rays=(m.rays[0], total - m.rays[0]), coarse_rays=report.share_rays, evals_full=report.evals_full), report


def _frame(r, pose, cus, n, outputs=LEAN):
    """Renders a frame of n rays; returns (reported, planned, the plan's report)."""
    H, W = _hw(n)
    fx, fy, cx, cy = O.intrinsics(H, W)
    r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR, outputs=outputs)
    return (_reports(r),) + _planned(r, cus, outputs, camera=(1, H, W))


@pytest.fixture()
def plain(renderer):
    yield renderer
    renderer.debug_set_decomposition(-1); renderer.debug_set_work_queue(-1)
    renderer.set_early_termination(0.0); renderer.set_shared_coarse(1); renderer.set_separate_passes(False)


@pytest.mark.parametrize("mode", [-1, 0, 1])
def test_plain_lean_frames(plain, pose, cus, mode):
    r = plain
    r.debug_set_work_queue(mode)
    seen = set()
    for dec in (-1, 0, 1, 2):
        r.debug_set_decomposition(dec)
        for n in _counts(cus, long=dec == -1):
            got, want, report = _frame(r, pose, cus, n)
            print(mode, dec, n, got)
            assert got == want, (mode, dec, n)
            assert r.last_ray_evaluations()[0] == report.evals_run == n * 24
            seen.add((want["plan"], bool(want["tail"]), want["side"], any(want["grid"])))
    # the cases are there: every plan; and, with the queue on, the tail path, the backfill beside it and a queued single launch
    assert {s[0] for s in seen} == {0, 1, 2}
    if mode == 1:
        assert {(2, True, True, True), (2, False, True, True), (0, False, False, True)} <= seen
    if mode == 0:
        assert all(s[1:] == (False, False, False) for s in seen)


def test_a_frame_that_is_not_lean(plain, pose, cus):
    r = plain
    r.debug_set_work_queue(1)
    for n in _counts(cus):
        got, want, report = _frame(r, pose, cus, n, LEAN + ("z_fine",))
        assert got == want and not got["tail"], n
    assert got["plan"] == 2 and got["side"]          # the last count: a hybrid plan whose second launch backfills the first


def test_render_rays_is_never_lean(plain, pose, cus):
    r = plain
    r.debug_set_work_queue(1)
    for n in _counts(cus):
        H, W = _hw(n)
        fx, fy, cx, cy = O.intrinsics(H, W)
        rays = r.create_rays(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR)
        r.render_rays(rays, outputs=LEAN)
        got = _reports(r)
        want, _ = _planned(r, cus, LEAN, n_rays=n)
        assert got == want and not got["tail"], n


def test_early_termination(plain, pose, cus):
    r = plain
    r.debug_set_work_queue(1)
    r.set_early_termination(0.01)
    for n in _counts(cus):
        got, want, report = _frame(r, pose, cus, n)
        assert got == want and got["grid"] == (0, 0) and report.need_evals and report.main.variant == 1, n
        assert r.last_ray_evaluations()[0] <= report.evals_full


def test_shared_coarse_pass(plain, pose, cus):
    r = plain
    r.debug_set_work_queue(1)
    r.set_shared_coarse(2)
    for n in _counts(cus):
        got, want, report = _frame(r, pose, cus, n)
        assert got == want and got["grid"] == (0, 0) and 0 < got["coarse_rays"] < n, n
        assert r.last_ray_evaluations()[0] == report.evals_run
        assert (report.share, report.coarse.variant, report.main.variant) == (1, 2, 2)


@pytest.mark.parametrize("outputs, kernels", [(LEAN, "sharing"), (LEAN + ("weights_coarse",), "full")])
def test_separate_passes(plain, pose, cus, outputs, kernels):
    r = plain
    r.debug_set_work_queue(1)
    r.set_separate_passes(True)
    for n in _counts(cus):
        got, want, report = _frame(r, pose, cus, n, outputs)
        assert got == want and got["grid"] == (0, 0) and got["coarse_rays"] == n, n
        assert r.last_ray_evaluations()[0] == report.evals_run == n * 24
        assert (report.share, report.full, report.table_elems) == ((1, 0, n * 8) if kernels == "sharing" else (0, 1, 0))


def test_separate_passes_with_the_coarse_weights_hook(plain, pose, cus):
    r = plain
    r.debug_set_work_queue(1)
    r.set_separate_passes(True)
    for n in _counts(cus):
        H, W = _hw(n)
        fx, fy, cx, cy = O.intrinsics(H, W)
        rays = r.create_rays(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR)
        weights = torch.rand(n, 8, generator=torch.Generator().manual_seed(n)) + 0.01
        r.render_rays(rays, outputs=LEAN, debug_coarse_weights=weights)
        got = _reports(r)
        want, report = _planned(r, cus, LEAN, n_rays=n, hooks=_lib.PLAN_HOOK_COARSE_WEIGHTS)
        assert got == want and got["coarse_rays"] == 0 and (report.full, report.coarse_launch) == (1, 0), n
