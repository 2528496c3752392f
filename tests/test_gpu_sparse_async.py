"""The asynchronous sparse frame on the GPU (include/nwe.h: nwe_render_sparse_async; the counted query kernels: csrc/nwe_mfma_query.h,
csrc/nwe_kernel_f32_counted.hip).

Everything is bit for bit against the synchronous call of the same context and arguments (which tests/test_gpu_sparse_fine.py holds to
the rule step by step): rgb, depth, acc, flags, every diagnostic and last_sparse_samples().  "Bit for bit" lets a NaN equal a NaN.
What can go wrong only here: the strided walk of the counted kernels (more packets than workgroups, a count that is no multiple of
the packet, fewer packets than workgroups, no packet at all), the chunk buffer reused by chunks that are queued without a wait (an
odd number of chunks, a chunk of one ray), calls queued back to back with nothing waited for in between, the scratch growing under
a call in flight, and the reports.
"""
import functools

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd.handler import NeRFReplicaInferenceHandler
from oracle import nerf_oracle as O
from tests import coarse_grid as B
from tests import radiance_grid as R
from tests import sparse_fine as SF

pytestmark = pytest.mark.gpu

LEAN = ("rgb", "depth", "acc")
DIAG = ("weights_coarse", "z_fine", "weights_grid", "selected", "raw_fine")
ALL = LEAN + DIAG


def _camera(H, W):
    fx, fy, cx, cy = O.intrinsics(H, W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=R.NEAR, far=R.FAR)


@functools.lru_cache(maxsize=None)
def _nets(name):
    """(coarse, fine) state dicts: "small" = s7's 4x128; "big" = 8x256; "big_novd" = 8x256 without view directions.  Shared: leave
    them unchanged."""
    S = nwe_amd.synthetic
    if name == "small":
        return B.scene("s7")[:2]
    if name == "big":
        return B.scene("big7")[:2]
    if name == "big_novd":
        return (S.thin_fog_output(S.make_state_dict(1000, 8, 256, use_view_dirs=False)),
                S.thin_fog_output(S.make_state_dict(1001, 8, 256, use_view_dirs=False), 0.5, B.G.X1_SPREAD))
    raise KeyError(name)


def _renderer(grid, ns, ni, sds=None):
    """Both networks and the grid behind them: an upload clears a grid."""
    sd_c, sd_f = sds or _nets("small")
    r = nwe_amd.Renderer(0)
    r.set_network(0, sd_c); r.set_network(1, sd_f)
    r.set_sampling(ns, ni)
    if grid is not None:
        r.set_radiance_grid(grid["values"], grid["lo"], grid["hi"])
    return r


def _sparse(r, poses, H, W, rows=None, outputs=ALL, **kw):
    return r.render_sparse(poses.numpy(), H, W, rows=rows, outputs=outputs, **_camera(H, W), **kw)


def _eq(a, b):
    if a.dtype != torch.float32:
        return torch.equal(a, b)
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) and torch.equal(torch.isnan(a), torch.isnan(b))


def _same(a, b, ctx, keys=ALL):
    for k in keys:
        assert _eq(a[k], b[k]), (ctx, k)
    assert int(a["flags"].item()) == int(b["flags"].item()), ctx


def _twin(r, poses, H, W, ctx, **kw):
    """The asynchronous call against the synchronous one of the same context and arguments; returns the asynchronous outputs."""
    want = _sparse(r, poses, H, W, **kw)
    count = r.last_sparse_samples()
    got = _sparse(r, poses, H, W, asynchronous=True, **kw)
    _same(got, want, ctx, tuple(kw.get("outputs", ALL)))
    assert r.last_sparse_samples() == count, ctx
    return got, count


def _busy(device, rounds=24):
    """Some tens of milliseconds of work on the current stream, so that what is queued behind it is certainly still in flight when the
    host makes its next call."""
    x = torch.ones(4096, 4096, device=device)
    for _ in range(rounds):
        x = (x @ x) * 1e-4
    return x


# ---- 1. chunking ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns,ni,precision,net", [
    (7, 6, "f32", "big"), (7, 6, "f16x3", "big"), (7, 6, "f32", "big_novd"), (7, 6, "f16x3", "big_novd"),
    (64, 128, "f32", "big"), (64, 128, "f16x3", "big"), (64, 128, "f32", "big_novd"), (64, 128, "f16x3", "big_novd"),
    (7, 6, "f16x3", "small")])
def test_chunks_queued_without_a_wait_give_the_synchronous_calls_bits(ns, ni, precision, net):
    """480 rays; chunks of 64, 1 and 100 rays are 8, 480 and 5 chunks: the buffer is reused, the count is odd, a chunk is one ray."""
    H, W = SF.H3, SF.W3
    poses, _ = B.G.E.frame_rays(H, W, 1)
    r = _renderer(R.grid("smooth" if ni else "random"), ns, ni, _nets(net))
    try:
        for min_weight in (-1.0, 1e-3, 2.0):
            for dilate in (0, 1):
                kw = dict(precision=precision, min_weight=min_weight, dilate=dilate)
                r.debug_set_sparse_chunk(0)
                want = _sparse(r, poses, H, W, **kw)
                count = r.last_sparse_samples()
                if min_weight < 0:
                    assert count == (H * W * (ns + ni),) * 2
                if min_weight == 2.0:
                    assert count[0] == 0
                for chunk in (0, 64, 1, 100):
                    r.debug_set_sparse_chunk(chunk)
                    got = _sparse(r, poses, H, W, asynchronous=True, **kw)
                    _same(got, want, (min_weight, dilate, chunk))
                    assert r.last_sparse_samples() == count, (min_weight, dilate, chunk)
    finally:
        r.close()


# ---- 2. the strided walk --------------------------------------------------------------------------------------------------------

def _threshold_for(weights, lo, hi, packet=128):
    """A min_weight that hits k samples (dilate 0) for some lo <= k < hi with k % packet != 0: the k-th largest weight must differ
    from the next one.  Returns (min_weight, k)."""
    w = np.sort(weights.reshape(-1))[::-1]
    assert not np.isnan(w).any()
    for k in range(lo, hi):
        if k % packet != 0 and w[k - 1] > w[k]:
            return float(w[k]), k
    raise AssertionError("no usable threshold")


def _rows_are_the_querys(r, poses, H, W, out, precision, view_dirs=True):
    sel = out["selected"].bool()
    rays = r.create_rays(poses.numpy(), H, W, **_camera(H, W))
    pts = torch.from_numpy(SF.points(rays.cpu().numpy(), out["z_fine"].cpu().numpy())).to(r.device)
    dirs = rays[:, 8:11].contiguous() if view_dirs else None
    q = r.query_points(pts, dirs, which=1, precision=precision, outputs=("raw",))["raw"]
    assert _eq(out["raw_fine"][sel], q[sel]), "selected rows"


@pytest.mark.parametrize("net", ["small", "big"])
def test_the_strided_walk_of_the_mfma_kernel(net):
    """2 560 rays at 3 + 1 in one chunk, forced steps 3: a capacity of 10 240 points, 80 packets on 27 workgroups."""
    H, W, ns, ni = 40, 64, 3, 1
    poses, _ = B.G.E.frame_rays(H, W, 1)
    lib = nwe_amd._lib.load()
    assert lib.nwe_debug_query_counted_grid(H * W * (ns + ni), 128, 3, 256) == 27
    r = _renderer(R.grid("smooth"), ns, ni, _nets(net))
    try:
        r.debug_set_query_steps(3)
        # everything selected: n = 10 240, a multiple of 128; every workgroup walks two or three packets
        got, count = _twin(r, poses, H, W, "all", precision="f16x3", min_weight=-1.0, dilate=0)
        assert count == (10240, 10240)
        _rows_are_the_querys(r, poses, H, W, got, "f16x3")
        # a count that is no multiple of 128 and below 27 x 128: a ragged last packet, and workgroups without a packet
        w = _sparse(r, poses, H, W, outputs=("weights_grid",), min_weight=2.0)["weights_grid"].cpu().numpy()
        min_weight, k = _threshold_for(w, 1000, 3000)
        got, count = _twin(r, poses, H, W, "ragged", precision="f16x3", min_weight=min_weight, dilate=0)
        print(f"strided walk, {net}: min_weight {min_weight:.6g} selects {count[0]} of {count[1]} samples")
        assert count[0] == k and count[0] % 128 != 0 and count[0] < 27 * 128
        _rows_are_the_querys(r, poses, H, W, got, "f16x3")
        # ... and above it: more packets than workgroups with a ragged end
        min_weight, k = _threshold_for(w, 27 * 128 + 200, 9000)
        got, count = _twin(r, poses, H, W, "ragged, more packets than workgroups", precision="f16x3", min_weight=min_weight, dilate=0)
        assert count[0] == k and count[0] % 128 != 0 and count[0] > 27 * 128
        _rows_are_the_querys(r, poses, H, W, got, "f16x3")
        # the automatic grid: one packet per workgroup
        r.debug_set_query_steps(0)
        _twin(r, poses, H, W, "automatic", precision="f16x3", min_weight=min_weight, dilate=1)
        _twin(r, poses, H, W, "automatic, f16x1", precision="f16x1", min_weight=min_weight, dilate=1)
    finally:
        r.close()


@pytest.mark.parametrize("net", ["small", "big_novd"])
def test_the_strided_walk_of_the_fp32_kernel(net):
    """480 rays at 3 + 1, 120 packets of 16, forced steps 7: 18 workgroups."""
    H, W, ns, ni = SF.H3, SF.W3, 3, 1
    poses, _ = B.G.E.frame_rays(H, W, 1)
    assert nwe_amd._lib.load().nwe_debug_query_counted_grid(H * W * (ns + ni), 16, 7, 256) == 18
    r = _renderer(R.grid("smooth"), ns, ni, _nets(net))
    try:
        r.debug_set_query_steps(7)
        vd = net != "big_novd"
        got, count = _twin(r, poses, H, W, "all", precision="f32", min_weight=-1.0, dilate=0)
        assert count == (1920, 1920)
        _rows_are_the_querys(r, poses, H, W, got, "f32", vd)
        w = _sparse(r, poses, H, W, outputs=("weights_grid",), min_weight=2.0)["weights_grid"].cpu().numpy()
        for lo, hi in ((100, 18 * 16), (18 * 16 + 30, 1800)):
            min_weight, k = _threshold_for(w, lo, hi, 16)
            got, count = _twin(r, poses, H, W, (lo, hi), precision="f32", min_weight=min_weight, dilate=0)
            assert count[0] == k and count[0] % 16 != 0 and lo <= count[0] < hi
            _rows_are_the_querys(r, poses, H, W, got, "f32", vd)
    finally:
        r.close()


# ---- 3. empty and near-empty counts ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("n_poses", [2, 3])
def test_chunks_with_nothing_selected_between_chunks_that_have_work(precision, n_poses):
    """The second pose is a hundred units outside the box; a chunk border lies on every pose border."""
    H, W, ns, ni = SF.H3, SF.W3, 7, 6
    poses, _ = B.G.E.frame_rays(H, W, 1)
    far = poses[:1].clone()
    far[0, 0, 3] += 100.0
    batch = torch.cat([poses[:1], far, poses[:1]][:n_poses])
    r = _renderer(R.grid("smooth"), ns, ni)
    try:
        for chunk in (240, 160, 96):                      # 2, 3 and 5 chunks a pose
            r.debug_set_sparse_chunk(chunk)
            got, count = _twin(r, batch, H, W, (n_poses, chunk), precision=precision, min_weight=1e-3, dilate=1)
            sel = got["selected"].view(n_poses, H * W, ns + ni)
            assert int(sel[1].sum()) == 0 and int(sel[0].sum()) > 0
            assert count[0] == int(sel.sum())
    finally:
        r.close()


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_a_frame_with_exactly_one_selected_sample(precision):
    """A row tile whose largest weight is unique (the frame is symmetric, so the whole frame's is not), min_weight = its second
    largest: n = 1 in one chunk and 0 in the others."""
    H, W, ns, ni = SF.H3, SF.W3, 7, 6
    poses, _ = B.G.E.frame_rays(H, W, 1)
    r = _renderer(R.grid("smooth"), ns, ni)
    try:
        w = _sparse(r, poses, H, W, outputs=("weights_grid",), min_weight=2.0)["weights_grid"].cpu().numpy().reshape(H, -1)
        tiles = [i for i in range(H) if np.sort(w[i])[-1] > np.sort(w[i])[-2]]
        assert tiles, "no row of the frame has a unique largest weight"
        row = tiles[0]
        min_weight = float(np.sort(w[row])[-2])
        for chunk in (0, 7):                                # one chunk, and three of which one has the sample
            r.debug_set_sparse_chunk(chunk)
            got, count = _twin(r, poses, H, W, chunk, rows=(row, row + 1), precision=precision, min_weight=min_weight, dilate=0)
            assert count == (1, W * (ns + ni)) and int(got["selected"].sum()) == 1
    finally:
        r.close()


# ---- 4. back to back ------------------------------------------------------------------------------------------------------------

def _fresh(grid, ns, ni, poses, H, W, **kw):
    """The synchronous frame of a fresh context."""
    f = _renderer(grid, ns, ni)
    try:
        out = _sparse(f, poses, H, W, **kw)
        return out, f.last_sparse_samples()
    finally:
        f.close()


def test_two_asynchronous_calls_with_nothing_waited_for_in_between():
    H, W, ns, ni = SF.H3, SF.W3, 7, 6
    poses, _ = B.G.E.frame_rays(H, W, 1)
    g = R.grid("smooth")
    a_kw, b_kw = dict(min_weight=1e-3, dilate=1), dict(min_weight=0.05, dilate=0)
    want_a, _ = _fresh(g, ns, ni, poses, H, W, **a_kw)
    want_b, count_b = _fresh(g, ns, ni, poses, H, W, **b_kw)
    assert not _eq(want_a["rgb"], want_b["rgb"])
    r = _renderer(g, ns, ni)
    try:
        r.debug_set_sparse_chunk(100)
        # one stream
        _busy(r.device)
        a = _sparse(r, poses, H, W, asynchronous=True, **a_kw)
        b = _sparse(r, poses, H, W, asynchronous=True, **b_kw)
        assert r.debug_last_sparse_host_waits() == 0
        _same(a, want_a, "first of two, one stream"); _same(b, want_b, "second of two, one stream")
        assert r.last_sparse_samples() == count_b
        # two streams: the second call waits on the device for the first, whose chunks use the same scratch
        streams = [torch.cuda.Stream(device=r.device) for _ in range(2)]
        outs = []
        for s, kw in zip(streams, (a_kw, b_kw)):
            with torch.cuda.stream(s):
                if not outs:
                    _busy(r.device)
                outs.append(_sparse(r, poses, H, W, asynchronous=True, **kw))
        for s in streams:
            s.synchronize()
        _same(outs[0], want_a, "first of two, two streams"); _same(outs[1], want_b, "second of two, two streams")
    finally:
        r.close()


@pytest.mark.parametrize("then", ["set_radiance_grid", "set_network", "set_sampling", "render_sparse"])
def test_an_asynchronous_call_followed_at_once_by_a_call_that_changes_what_it_reads(then):
    H, W, ns, ni = SF.H3, SF.W3, 7, 6
    poses, _ = B.G.E.frame_rays(H, W, 1)
    g, other = R.grid("smooth"), R.grid("random")
    kw = dict(min_weight=1e-3, dilate=1)
    want, count = _fresh(g, ns, ni, poses, H, W, **kw)
    r = _renderer(g, ns, ni)
    try:
        r.debug_set_sparse_chunk(100)
        _busy(r.device)
        got = _sparse(r, poses, H, W, asynchronous=True, **kw)
        if then == "set_radiance_grid":
            r.set_radiance_grid(other["values"], other["lo"], other["hi"])
        elif then == "set_network":
            r.set_network(1, _nets("big")[1])
        elif then == "set_sampling":
            r.set_sampling(5, 3)
        else:
            sync_kw = dict(min_weight=0.05, dilate=0)
            second = _sparse(r, poses, H, W, **sync_kw)
            assert r.debug_last_sparse_host_waits() == 6
            _same(second, _fresh(g, ns, ni, poses, H, W, **sync_kw)[0], "the synchronous call behind it")
        _same(got, want, then)
        if then != "render_sparse":
            assert r.last_sparse_samples() == count
    finally:
        r.close()


# ---- 5. scratch growth ----------------------------------------------------------------------------------------------------------

def test_the_scratch_grows_under_a_call_in_flight():
    ns, ni = 7, 6
    g = R.grid("smooth")
    kw = dict(min_weight=1e-3, dilate=1)
    small_p, _ = B.G.E.frame_rays(R.H2, R.W2, 1)
    large_p, _ = B.G.E.frame_rays(SF.H3, SF.W3, 1)
    want_small, _ = _fresh(g, ns, ni, small_p, R.H2, R.W2, **kw)
    want_large, _ = _fresh(g, ns, ni, large_p, SF.H3, SF.W3, **kw)
    r = _renderer(g, ns, ni)
    try:
        _busy(r.device)
        first = _sparse(r, small_p, R.H2, R.W2, asynchronous=True, **kw)
        assert r.debug_last_sparse_host_waits() == 0
        large = _sparse(r, large_p, SF.H3, SF.W3, asynchronous=True, **kw)       # the scratch of 144 rays does not hold 480
        waits = r.debug_last_sparse_host_waits()
        last = _sparse(r, small_p, R.H2, R.W2, asynchronous=True, **kw)
        assert r.debug_last_sparse_host_waits() == 0
        print(f"scratch growth: the growing call waited {waits} time(s)")
        assert waits >= 1
        _same(first, want_small, "small, before"); _same(large, want_large, "large"); _same(last, want_small, "small, after")
    finally:
        r.close()


# ---- 6. no host wait ------------------------------------------------------------------------------------------------------------

def test_a_warmed_asynchronous_call_makes_no_host_wait():
    H, W, ns, ni = SF.H3, SF.W3, 7, 6
    poses, _ = B.G.E.frame_rays(H, W, 1)
    r = _renderer(R.grid("smooth"), ns, ni)
    try:
        assert r.debug_last_sparse_host_waits() is None
        r.debug_set_sparse_chunk(100)                     # 5 chunks
        _sparse(r, poses, H, W, asynchronous=True)        # the warm-up: the scratch, the tally, the pinned word
        _busy(r.device)
        _sparse(r, poses, H, W, asynchronous=True)
        assert r.debug_last_sparse_host_waits() == 0
        _sparse(r, poses, H, W)
        assert r.debug_last_sparse_host_waits() == 6      # a read-back per chunk and the wait at the end
    finally:
        r.close()


# ---- 7. reports -----------------------------------------------------------------------------------------------------------------

def test_an_asynchronous_call_moves_no_other_report():
    sd_c, sd_f, cfg, poses, _, H, W = B.scene("s7")
    g = R.grid("random")
    r = _renderer(None, cfg.n_samples, cfg.n_importance)
    try:
        cam = _camera(H, W)
        first = r.render(poses.numpy(), H, W, precision="f16x3", **cam)
        r.query_points(torch.zeros(5, 3, device=r.device), None, outputs=("sigma",))
        r.set_radiance_grid(g["values"], g["lo"], g["hi"])
        r.render_grid(poses.numpy(), H, W, **cam)
        reports = lambda: (r.last_kernel_ms(), r.last_launch_parts(), r.last_query_ms(), r.last_grid_ms(), r.last_ray_evaluations(),
                           r.debug_last_plan(), r.last_coarse_launch())
        before = reports()
        assert r.last_sparse_ms() is None and r.last_sparse_samples() is None
        r.debug_set_sparse_chunk(100)
        got = _sparse(r, poses, H, W, asynchronous=True, min_weight=0.02, dilate=1)
        ms = r.last_sparse_ms()
        assert ms is not None and ms > 0 and reports() == before and before[0] > 0
        sel = int(got["selected"].sum())
        assert r.last_sparse_samples() == (sel, H * W * (cfg.n_samples + cfg.n_importance)) and 0 < sel
        assert r.last_sparse_samples() == (sel, H * W * (cfg.n_samples + cfg.n_importance))      # asked twice
        second = r.render(poses.numpy(), H, W, precision="f16x3", **cam)
        _same(first, second, "the render after an asynchronous sparse frame", LEAN)
        assert r.last_sparse_ms() == ms
        empty = _sparse(r, poses, H, W, rows=(5, 5), asynchronous=True)          # zero rays: NWE_OK, nothing moves
        assert tuple(empty["rgb"].shape) == (0, 3) and int(empty["flags"].item()) == 0 and r.last_sparse_ms() == ms
    finally:
        r.close()


# ---- 8. the end-to-end contract -------------------------------------------------------------------------------------------------

def test_everything_selected_is_the_render_under_a_baked_coarse_pass():
    """tests/test_gpu_sparse_fine.py holds the synchronous call to this; the asynchronous call inherits it through the counted kernel."""
    sd_c, _, cfg, poses, _, H, W = B.scene("s7")
    g = R.grid("smooth")
    r = _renderer(g, cfg.n_samples, cfg.n_importance, (sd_c, SF.room_net()))
    try:
        r.debug_set_sparse_chunk(100)
        out = _sparse(r, poses, H, W, outputs=LEAN + ("selected",), precision="f16x3", min_weight=-1.0, dilate=0, asynchronous=True)
        assert bool(out["selected"].bool().all())
        r.set_coarse_grid(np.ascontiguousarray(g["values"][..., 3]), g["lo"], g["hi"])
        ref = r.render(poses.numpy(), H, W, precision="f16x3", outputs=LEAN, **_camera(H, W))
        _same(out, ref, "min_weight -1 against the baked coarse render", LEAN)
    finally:
        r.close()


# ---- 9. the handler -------------------------------------------------------------------------------------------------------------

def test_the_handler_draws_the_same_frame_with_the_option():
    sd_c = B.scene("s7")[0]
    opt = {"min_weight": 1e-3, "dilate": 1}
    box = {"lo": SF.ROOM_LO, "hi": SF.ROOM_HI, "resolution": 16, "view_dir": (0.0, 0.0, 1.0)}
    init, coord = nwe_amd.COORD(x=0.0, y=-0.5, z=-0.76, pitch=-90.0), nwe_amd.COORD(yaw=-30.0)
    frames, counts = [], []
    for sparse_async in (False, True):
        h = NeRFReplicaInferenceHandler("office_tokyo", "unused", precision="f16x3", sparse_fine=opt, radiance_grid=box,
                                        sparse_async=sparse_async)
        h.set_sampling(7, 6)
        h.initialize_models(state_dicts=(sd_c, SF.room_net()))
        try:
            frames.append(h.render_coordinates(init, coord))
            counts.append(h.last_sparse_samples())
            waits = h.renderer.debug_last_sparse_host_waits()
            assert (waits == 0) if sparse_async else (waits >= 2)
        finally:
            h.renderer.close()
    assert frames[0].dtype == np.uint8 and np.array_equal(frames[0], frames[1]) and counts[0] == counts[1] and 0 < counts[0][0] < counts[0][1]
