"""Ray generation over the legal camera domain, case by case from tests/camera_domain.py, through every entry point that takes
a camera: nwe_create_rays, nwe_render (the fp32 kernel's load_ray, the MFMA kernels' seed_ray + make_ray in both
decompositions and under the hybrid plan's second launch) and nwe_render_tiled.

Every comparison is BITWISE, through an int32 view, so that zero signs count; no tolerance, no ray left out.  The rays are
compared with the reference's recorded ones (tests/golden/cameras.npz); a render from the pose is compared with the same
kernel's render of the reference's rays (nwe_render_rays), which only bit-identical origins, directions and view directions can
equal.  Networks: 4x128, a thin-fog coarse and a random fine network, 8 + 8 samples - small, and both passes and the sampler
run - with and without view directions.

fx == 0 or fy == 0 is refused by all three entry points before anything is queued."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib, dist, synthetic
from tests import camera_domain as CD

pytestmark = pytest.mark.gpu

NS, NI = 8, 8
LEAN = ("rgb", "depth", "acc")
FULL = LEAN + ("raw_coarse", "raw_fine", "z_fine")
# (name, precision, forced decomposition or None, outputs)
MODES = [("f32", "f32", None, FULL),
         ("f16x3-packets-lean", "f16x3", 0, LEAN), ("f16x3-packets-full", "f16x3", 0, FULL),
         ("f16x3-split-lean", "f16x3", 1, LEAN), ("f16x3-split-full", "f16x3", 1, FULL),
         ("f16x1", "f16x1", None, FULL)]
MODE_NAMES = [m[0] for m in MODES]
BY_MODE = {m[0]: m for m in MODES}


def _networks(view_dirs):
    if view_dirs:
        return synthetic.thin_fog(synthetic.make_state_dict(3100, 4, 128)), synthetic.make_state_dict(3101, 4, 128)
    return (synthetic.thin_fog_output(synthetic.make_state_dict(3102, 4, 128, use_view_dirs=False)),
            synthetic.make_state_dict(3103, 4, 128, use_view_dirs=False))


def _setup(r, view_dirs, ns=NS, ni=NI):
    sd_c, sd_f = _networks(view_dirs)
    r.set_network(0, sd_c)
    r.set_network(1, sd_f)
    r.set_sampling(ns, ni)
    return r


@pytest.fixture(scope="module")
def renderers():
    """{view_dirs: renderer}: one context with view directions (11-column rays), one without (8 columns)."""
    rs = {vd: _setup(nwe_amd.Renderer(0), vd) for vd in (True, False)}
    yield rs
    for r in rs.values():
        r.close()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "cameras.npz"))


def _reference_rays(c, gold, view_dirs=True):
    """The reference's rays of the case's row window: the matching slice of the recorded whole frames."""
    full = gold[f"rays_{c.name}"]
    return CD.window_of(full if view_dirs else np.ascontiguousarray(full[..., :8]), c)


def _differences(got, ref, keys, what):
    out = []
    for k in keys:
        a, b = CD.bits(got[k]), CD.bits(ref[k])
        if a.shape != b.shape:
            out.append(f"{what} {k}: shape {a.shape} != {b.shape}")
        elif not np.array_equal(a, b):
            rays = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(-1))
            out.append(f"{what} {k}: {rays.size} of {a.shape[0]} rays differ, first {rays[:4].tolist()}")
    return out


def _render_pair(r, c, rays, precision, decomposition, outputs):
    """(render from the pose, render of the given rays) in one mode."""
    r.debug_set_decomposition(-1 if decomposition is None else decomposition)
    try:
        a = r.render(c.poses, c.H, c.W, rows=c.rows, precision=precision, outputs=outputs, **c.camera())
        plan_a = r.debug_last_plan()
        b = r.render_rays(torch.from_numpy(rays).cuda(), precision=precision, outputs=outputs)
        plan_b = r.debug_last_plan()
        torch.cuda.synchronize()
    finally:
        r.debug_set_decomposition(-1)
    if decomposition is not None:
        assert plan_a == decomposition and plan_b == decomposition, (plan_a, plan_b)
    return a, b


# ------------------------------------------------------------------------------------------------------------------------
# 1. nwe_create_rays
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CD.NAMES)
def test_create_rays_equals_the_reference(name, renderers, gold):
    c = CD.BY_NAME[name]
    r = renderers[True]
    for vd in (True, False):
        ref = _reference_rays(c, gold, vd)
        got = r.create_rays(c.poses, c.H, c.W, rows=c.rows, use_view_dirs=vd, **c.camera()).cpu().numpy()
        assert got.shape == ref.shape == (c.n_rays, 11 if vd else 8)
        bad = np.argwhere(CD.bits(got) != CD.bits(ref))
        assert bad.size == 0, (name, vd, f"{len(set(bad[:, 0].tolist()))} rays, columns {sorted(set(bad[:, 1].tolist()))}",
                               [(int(i), int(j), float(got[i, j]), float(ref[i, j])) for i, j in bad[:4]])
    if c.rows is not None:       # the window is the matching slice of the whole frames
        whole = r.create_rays(c.poses, c.H, c.W, **c.camera()).cpu().numpy().reshape(c.n_poses, c.H * c.W, 11)
        assert CD.same_bits(whole, gold[f"rays_{name}"])


# ------------------------------------------------------------------------------------------------------------------------
# 2. nwe_render from the pose == nwe_render_rays on the reference's rays, every kernel mode
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("name", CD.NAMES)
def test_render_from_pose_equals_render_of_reference_rays(name, mode, renderers, gold):
    c = CD.BY_NAME[name]
    _, precision, decomposition, outputs = BY_MODE[mode]
    problems = []
    for vd in (True, False):
        a, b = _render_pair(renderers[vd], c, _reference_rays(c, gold, vd), precision, decomposition, outputs)
        assert a["rgb"].shape == (c.n_rays, 3)
        problems += _differences(a, b, outputs, f"{name} {mode} {'view dirs' if vd else 'no view dirs'}")
    assert not problems, problems


def test_garbage_bottom_row_equals_its_clean_twin(renderers):
    g, clean = (CD.BY_NAME[n] for n in CD.GARBAGE_PAIR)
    problems = []
    for vd in (True, False):
        r = renderers[vd]
        ra, rb = (r.create_rays(x.poses, x.H, x.W, **x.camera()) for x in (g, clean))
        problems += _differences({"rays": ra}, {"rays": rb}, ("rays",), "create_rays")
        for mode, precision, decomposition, outputs in MODES:
            r.debug_set_decomposition(-1 if decomposition is None else decomposition)
            try:
                a, b = (r.render(x.poses, x.H, x.W, precision=precision, outputs=outputs, **x.camera()) for x in (g, clean))
                torch.cuda.synchronize()
            finally:
                r.debug_set_decomposition(-1)
            problems += _differences(a, b, outputs, f"{mode} {'view dirs' if vd else 'no view dirs'}")
    assert not problems, problems


# ------------------------------------------------------------------------------------------------------------------------
# 3. nwe_render_tiled: three contexts on one device
# ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiled():
    t = _setup(nwe_amd.TiledRenderer([0, 0, 0]), True)
    yield t
    t.close()


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("name", CD.TILED_NAMES)
def test_tiled_frame_equals_the_single_context_frame(name, precision, tiled, renderers):
    c = CD.BY_NAME[name]
    tiles = dist.shard_rows(c.H, 3)
    assert len({b - a for a, b in tiles}) == 2, tiles                         # H % 3 != 0: tiles of two different heights
    got = tiled.render(c.poses, c.H, c.W, precision=precision, outputs=LEAN, **c.camera())
    assert tiled.last_tiled
    one = renderers[True].render(c.poses, c.H, c.W, precision=precision, outputs=LEAN, **c.camera())
    torch.cuda.synchronize()
    assert got["rgb"].shape == (c.n_poses * c.H * c.W, 3)
    problems = _differences(got, one, LEAN, f"{name} {precision} tiles {tiles}")
    assert not problems, problems
    assert int(got["flags"].item()) == int(one["flags"].item())


# ------------------------------------------------------------------------------------------------------------------------
# 4. the hybrid plan: the second launch starts inside a row of the last pose
# ------------------------------------------------------------------------------------------------------------------------

def test_hybrid_plan_decodes_pose_row_and_column():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = CD.hybrid_case(cus)
    first = cus * CD.RAYS_PER_WORKGROUP
    per_pose = (c.window[1] - c.window[0]) * c.W
    assert first < c.n_rays < 2 * first and first // per_pose == 2 and (first % per_pose) % c.W != 0
    rays = CD.oracle_rays(c)                                                 # the live oracle: the frame is sized at run time
    r = _setup(nwe_amd.Renderer(0), True, 4, 4)
    try:
        got = r.create_rays(c.poses, c.H, c.W, rows=c.rows, **c.camera())
        assert CD.same_bits(got, rays), "create_rays on the hybrid frame"
        got8 = r.create_rays(c.poses, c.H, c.W, rows=c.rows, use_view_dirs=False, **c.camera())
        assert CD.same_bits(got8, CD.oracle_rays(c, False))
        rays_dev = torch.from_numpy(rays).cuda()
        problems = []
        for outputs in (LEAN, FULL):
            tag = "lean" if outputs is LEAN else "full"
            ref = r.render_rays(rays_dev, precision="f16x3", outputs=outputs)
            res = {}
            for plan in (0, 1, 2):
                r.debug_set_decomposition(plan)
                res[plan] = r.render(c.poses, c.H, c.W, rows=c.rows, precision="f16x3", outputs=outputs, **c.camera())
                assert r.debug_last_plan() == plan
                if plan == 2:
                    parts = r.last_launch_parts()
                    assert [n for _, n in parts] == [first, c.n_rays - first], parts
            r.debug_set_decomposition(-1)
            torch.cuda.synchronize()
            for plan in (0, 1, 2):
                problems += _differences(res[plan], ref, outputs, f"hybrid frame {tag}, plan {plan} against render_rays")
        assert not problems, problems
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. fx == 0 or fy == 0: refused before anything is queued
# ------------------------------------------------------------------------------------------------------------------------

SENTINEL = -12345.0
ZEROS = [("fx", 0.0), ("fx", -0.0), ("fy", 0.0), ("fy", -0.0)]


def _timing(r):
    return r.last_kernel_ms(), r.last_launch_parts()


def _camera_args(c, which, zero):
    cam = dict(c.camera())
    cam[which] = zero
    return [cam[k] for k in ("fx", "fy", "cx", "cy", "near", "far")]


def _fresh_frame(c, precision="f16x3"):
    r = _setup(nwe_amd.Renderer(0), True)
    try:
        out = r.render(c.poses, c.H, c.W, precision=precision, outputs=FULL, **c.camera())
        torch.cuda.synchronize()
        return {k: out[k].clone() for k in FULL}
    finally:
        r.close()


@pytest.mark.parametrize("which,zero", ZEROS, ids=[f"{w}={z}" for w, z in ZEROS])
def test_zero_focal_length_is_refused_by_create_rays(which, zero):
    c = CD.BY_NAME["focal-10x14"]
    r = _setup(nwe_amd.Renderer(0), True)
    try:
        before = r.render(c.poses, c.H, c.W, outputs=FULL, **c.camera())
        torch.cuda.synchronize()
        timing = _timing(r)
        buf = torch.full((c.n_rays, 11), SENTINEL, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        rc = r._lib.nwe_create_rays(r._ctx, c.poses.ctypes.data, c.n_poses, c.H, c.W, *_camera_args(c, which, zero), 0, c.H,
                                    buf.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == _lib.NWE_ERR_INVALID, rc
        assert b"non-zero" in r._lib.nwe_last_error(r._ctx)
        assert bool((buf == SENTINEL).all()), "a refused nwe_create_rays wrote rays"
        assert _timing(r) == timing
        with pytest.raises(ValueError, match="non-zero"):                    # and through the wrapper
            r.create_rays(c.poses, c.H, c.W, **{**c.camera(), which: zero})
        after = r.render(c.poses, c.H, c.W, outputs=FULL, **c.camera())
        torch.cuda.synchronize()
        fresh = _fresh_frame(c)
        assert not _differences(after, fresh, FULL, "after the refusal") and not _differences(before, fresh, FULL, "before it")
    finally:
        r.close()


@pytest.mark.parametrize("which,zero", ZEROS, ids=[f"{w}={z}" for w, z in ZEROS])
def test_zero_focal_length_is_refused_by_render(which, zero):
    c = CD.BY_NAME["focal-10x14"]
    r = _setup(nwe_amd.Renderer(0), True)
    try:
        r.render(c.poses, c.H, c.W, outputs=LEAN, **c.camera())
        torch.cuda.synchronize()
        timing = _timing(r)
        for precision in ("f16x3", "f32"):
            with torch.cuda.device(r.device):
                o, res = r._alloc(c.n_rays, FULL)
                for k in FULL:
                    res[k].fill_(SENTINEL)
                torch.cuda.synchronize()
                rc = r._lib.nwe_render(r._ctx, c.poses.ctypes.data, c.n_poses, c.H, c.W, *_camera_args(c, which, zero), 0, c.H,
                                       _lib.PRECISIONS[precision], C.byref(o), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert rc == _lib.NWE_ERR_INVALID, rc
            assert b"non-zero" in r._lib.nwe_last_error(r._ctx)
            assert all(bool((res[k] == SENTINEL).all()) for k in FULL) and int(res["flags"].item()) == 0
            assert _timing(r) == timing
        after = r.render(c.poses, c.H, c.W, outputs=FULL, **c.camera())
        torch.cuda.synchronize()
        assert not _differences(after, _fresh_frame(c), FULL, "after the refusal")
    finally:
        r.close()


@pytest.mark.parametrize("which,zero", ZEROS, ids=[f"{w}={z}" for w, z in ZEROS])
def test_zero_focal_length_is_refused_by_render_tiled(which, zero):
    c = CD.BY_NAME["focal-10x14"]
    t = _setup(nwe_amd.TiledRenderer([0, 0, 0]), True)
    try:
        before = t.render(c.poses, c.H, c.W, outputs=LEAN, **c.camera())
        torch.cuda.synchronize()
        timing = [_timing(p) for p in t.parts]
        n = c.n_poses * c.H * c.W
        bufs = {k: torch.full((n, 3) if k == "rgb" else (n,), SENTINEL, dtype=torch.float32, device="cuda") for k in LEAN}
        flags = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = t._lib.nwe_render_tiled(t._ctxs, len(t.parts), c.poses.ctypes.data, c.n_poses, c.H, c.W, *_camera_args(c, which, zero),
                                     _lib.PRECISIONS["f16x3"], bufs["rgb"].data_ptr(), bufs["depth"].data_ptr(), bufs["acc"].data_ptr(),
                                     flags.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == _lib.NWE_ERR_INVALID, rc
        assert t._lib.nwe_last_error(t.parts[0]._ctx) == b"fx and fy must be non-zero"
        assert all(bool((bufs[k] == SENTINEL).all()) for k in LEAN) and int(flags.item()) == 0
        assert [_timing(p) for p in t.parts] == timing
        with pytest.raises(ValueError, match="non-zero"):
            t.render(c.poses, c.H, c.W, outputs=LEAN, **{**c.camera(), which: zero})
        after = t.render(c.poses, c.H, c.W, outputs=LEAN, **c.camera())
        torch.cuda.synchronize()
        fresh = _fresh_frame(c)
        assert not _differences(after, fresh, LEAN, "after the refusal") and not _differences(before, fresh, LEAN, "before it")
    finally:
        t.close()
