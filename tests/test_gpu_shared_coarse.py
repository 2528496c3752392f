"""The coarse pass shared by k x k pixel blocks on the GPU (include/nwe.h: nwe_set_shared_coarse; the kernels' part:
csrc/nwe_mfma_render.h, csrc/nwe_kernel_f32.hip).

The rule is checked bit for bit against code that exists without it: a ray's shared frame is its own fine pass on the depths
the ordinary render gives its representative (render_rays with z_fine out, then render_rays with fine_depths = Z[rep]).  The
oracle's version of the same (tests/shared_coarse.py) is compared at the project's parity tolerances on scenes where it
reproduces itself (tests/test_shared_coarse_host.py).  Frames are a few hundred rays.
"""
import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import synthetic
from oracle import nerf_oracle as O
from tests import early_termination as E
from tests import mode_domain as M
from tests import shared_coarse as SC

pytestmark = pytest.mark.gpu

LEAN = ("rgb", "depth", "acc")
TOL = {"rgb": 1e-4, "depth": 1e-4 * E.FAR, "acc": 1e-4}
FRAMES = {"7x19x2": (7, 19, 2), "12x64": (12, 64, 1)}
# name -> (depth, width, view directions): the bench's kind of raw random networks, the roughest weights there are; "4x128",
# "8x256", "4x128-noview" and every other shape the sharing kernels are built for
NETS = M.NETS


def _nets(kind, seed=1000):
    D, W, view = NETS[kind]
    return tuple(synthetic.make_state_dict(seed + i, D, W, use_view_dirs=view) for i in (0, 1))


def _renderer(kind="4x128", ns=64, ni=128, k=1, devices=None, fold=True):
    r = nwe_amd.TiledRenderer(devices) if devices else nwe_amd.Renderer(0)
    if not fold:
        r.debug_set_fold(False)
    sd_c, sd_f = _nets(kind)
    r.set_network(0, sd_c); r.set_network(1, sd_f)
    r.set_sampling(ns, ni)
    if k != 1:
        r.set_shared_coarse(k)
    return r


def _camera(H, W):
    fx, fy, cx, cy = O.intrinsics(H, W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=E.NEAR, far=E.FAR)


def _poses(n_poses):
    return E.frame_rays(1, 1, n_poses)[0].numpy()


def _frame(r, H, W, n_poses=1, precision="f16x3", rows=None, outputs=LEAN, poses=None):
    return r.render(_poses(n_poses) if poses is None else poses, H, W, rows=rows, precision=precision, outputs=outputs, **_camera(H, W))


def _same(a, b, ctx):
    for key in LEAN:
        assert torch.equal(torch.nan_to_num(a[key], nan=-7.0), torch.nan_to_num(b[key], nan=-7.0)), (ctx, key)
    assert int(a["flags"].item()) == int(b["flags"].item()), (ctx, hex(int(a["flags"].item())), hex(int(b["flags"].item())))


FINE_FLAGS = 0x30F      # bits 0-3 (rgb / depth / acc / disp of the frame), 8 (raw), 9 (z_std); 4-7 are the coarse pass's


def _same_as_expected(got, want, ctx):
    """Outputs bit for bit, and the flags of what the rule covers: the bits of the frame's own outputs are equal; the coarse
    bits are the expected render's alone - its rays ran a coarse pass of their own, which a shared frame does not have
    (include/nwe.h: never raised)."""
    _same(got, dict(want, flags=want["flags"] & FINE_FLAGS), ctx)
    assert int(got["flags"].item()) & 0xF0 == 0, (ctx, hex(int(got["flags"].item())))


def _expected(r, H, W, n_poses, k, precision, view=True):
    """What the rule says, from entry points that exist without it: (a) the ordinary render's fine depths Z of the frame's
    rays, (b) every ray's fine pass on Z[rep].  The context must have k = 1 while this runs."""
    return M.expected_shared(r, _poses(n_poses), H, W, k, precision, view, _camera(H, W))


# ---- 1. the rule, bit for bit -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("kind,ns,ni,precision,white", [
    ("4x128", 64, 128, "f16x3", False),
    ("8x256", 64, 128, "f16x3", True),
    ("4x128", 7, 6, "f16x3", True),
    ("4x128-noview", 64, 128, "f16x3", False),
    ("4x128", 64, 128, "f16x1", True),
    ("8x256", 7, 6, "f16x1", False),
    ("4x128-noview", 7, 6, "f16x1", True),
    ("4x128", 64, 128, "f32", False),
    ("4x128-noview", 7, 6, "f32", True),
])
def test_shared_frame_is_each_rays_fine_pass_on_its_representatives_depths(frame, kind, ns, ni, precision, white):
    """7 x 19 with 2 poses: odd in both directions, so the last block row and column are cut and their representatives
    clamped to the image edge; 12 x 64: several workgroups.  k = 2, 3, 4, both decompositions, no tolerance in rgb, depth,
    acc and the flag bits of the frame's own outputs."""
    H, W, n_poses = FRAMES[frame]
    r = _renderer(kind, ns, ni)
    try:
        r.set_white_background(white)
        for k in (2, 3, 4):
            r.set_shared_coarse(1)
            want = _expected(r, H, W, n_poses, k, precision, NETS[kind][2])
            plain = _frame(r, H, W, n_poses, precision)
            r.set_shared_coarse(k)
            for mode in ((0, 1) if precision != "f32" else (-1,)):
                r.debug_set_decomposition(mode)
                got = _frame(r, H, W, n_poses, precision)
                _same_as_expected(got, want, (frame, kind, ns, ni, precision, white, k, mode))
                assert r.last_coarse_launch()[1] == SC.n_rep(H, W, k, 0, H, n_poses)
            r.debug_set_decomposition(-1)
            assert not torch.equal(got["rgb"], plain["rgb"]), "the rule changes the frame"
    finally:
        r.close()


# ---- 2. against the oracle ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["thin", "mixed"])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_parity_with_the_oracles_shared_reference(name, precision):
    """rgb 1e-4, depth 1e-4 * far, acc 1e-4 on every ray, k = 2 and 4."""
    sd_c, sd_f, cfg, poses, _, _ = E.scene(name)
    H, W = E.SCENES[name][6:8]
    r = nwe_amd.Renderer(0)
    try:
        r.set_network(0, sd_c); r.set_network(1, sd_f)
        r.set_sampling(cfg.n_samples, cfg.n_importance)
        for k in (2, 4):
            ref = SC.shared_reference(name, k)
            r.set_shared_coarse(k)
            out = _frame(r, H, W, precision=precision, poses=poses.numpy())
            assert int(out["flags"].item()) & 0x7 == 0
            errs = {}
            for key in LEAN:
                err = (out[key].cpu() - ref[key]).abs()
                errs[key] = float(err.max())
                print(f"{name} {precision} k {k} {key}: max err {errs[key]:.2e} (tol {TOL[key]:.0e})")
            for key in LEAN:
                assert errs[key] <= TOL[key], (name, precision, k, key)
    finally:
        r.close()


# ---- 3. invariance ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_row_tiles_pose_batches_and_context_tiles_equal_the_frame(precision, k):
    """Blocks sit on the grid of the whole image: rows [0, 3) [3, 6) [6, 7) of the 7 x 19 frame cut through blocks (their
    representatives lie outside the tile), the poses rendered apart and the tiles of two and three contexts all give the
    frame's bits."""
    H, W = 7, 19
    r = _renderer(k=k)
    tiled = [_renderer(k=k, devices=[0] * n) for n in (2, 3)]
    try:
        whole = _frame(r, H, W, 2, precision)
        parts = [_frame(r, H, W, 2, precision, rows=rows) for rows in ((0, 3), (3, 6), (6, 7))]
        for key in LEAN:
            w = whole[key].reshape((2, H, W) + tuple(whole[key].shape[1:]))
            rows = torch.cat([p[key].reshape((2, -1, W) + tuple(p[key].shape[1:])) for p in parts], 1)
            assert torch.equal(w, rows), (precision, k, key, "row tiles")
        for p in range(2):
            one = _frame(r, H, W, precision=precision, poses=_poses(2)[p])
            for key in LEAN:
                assert torch.equal(one[key], whole[key][p * H * W:(p + 1) * H * W]), (precision, k, key, "pose", p)
        for t in tiled:
            out = _frame(t, H, W, 2, precision)
            assert t.last_tiled and all(p.shared_coarse == k for p in t.parts)
            assert all(p.last_coarse_launch() is not None for p in t.parts)
            _same(out, whole, (precision, k, "context tiles", len(t.parts)))
    finally:
        r.close()
        for t in tiled:
            t.close()


@pytest.mark.parametrize("precision", ["f16x3", "f16x1"])
def test_forced_plans_agree_bit_for_bit(precision):
    """Packets, sample split and the hybrid plan force both launches.  The small frame: every plan on a ragged count; 300 x 200
    at 4x128: one full round of packet workgroups and a sample-split rest in the consumer."""
    r = _renderer(k=3)
    try:
        for H, W in ((7, 19), (200, 300)):
            res = {}
            for mode in (0, 1, 2):
                r.debug_set_decomposition(mode)
                res[mode] = _frame(r, H, W, precision=precision)
                assert r.debug_last_plan() == mode
            _same(res[0], res[1], (precision, H, W, "0 vs 1"))
            _same(res[0], res[2], (precision, H, W, "0 vs 2"))
            r.debug_set_decomposition(-1)
            _same(res[0], _frame(r, H, W, precision=precision), (precision, H, W, "0 vs the launcher's choice"))
    finally:
        r.close()


# ---- 4. off means off ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f16x1", "f32"])
def test_off_is_a_context_that_never_heard_of_it(precision):
    """k = 1 after k = 4, and k = 4 without importance samples (no pass to share), render the bits of a fresh context, report
    the full evaluation count and no coarse launch."""
    H, W = 7, 19
    r, fresh = _renderer(k=4), _renderer()
    try:
        on = _frame(r, H, W, 2, precision)
        assert r.last_coarse_launch() is not None
        r.set_shared_coarse(1)
        off, ref = _frame(r, H, W, 2, precision), _frame(fresh, H, W, 2, precision)
        _same(off, ref, (precision, "k back to 1"))
        assert not torch.equal(on["rgb"], off["rgb"])
        assert r.last_coarse_launch() is None and fresh.last_coarse_launch() is None
        assert r.last_ray_evaluations() == fresh.last_ray_evaluations() == SC.evaluations(H, W, 1, 0, H, 2, 64, 128)
        r.set_shared_coarse(4)
        for x in (r, fresh):
            x.set_sampling(32, 0)
        _same(_frame(r, H, W, 2, precision), _frame(fresh, H, W, 2, precision), (precision, "k = 4, n_importance == 0"))
        assert r.shared_coarse == 4 and r.last_coarse_launch() is None
        assert r.last_ray_evaluations() == fresh.last_ray_evaluations() == (2 * H * W * 32,) * 2
    finally:
        r.close(); fresh.close()


# ---- 5. counts ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_counts_and_times_of_the_two_launches(precision):
    """The frame and the unaligned tile rows [3, 6) of 7 x 19 with two poses: executed / full evaluations and the producer's
    rays are the helper's arithmetic; the whole spans the producer and the consumer's parts."""
    H, W = 7, 19
    for k in (2, 4):
        r = _renderer(k=k)
        try:
            for rows in ((0, H), (3, 6), (4, 7)):
                _frame(r, H, W, 2, precision, rows=rows)
                assert r.last_ray_evaluations() == SC.evaluations(H, W, k, rows[0], rows[1], 2, 64, 128), (k, rows)
                ms_coarse, rays_coarse = r.last_coarse_launch()
                assert rays_coarse == SC.n_rep(H, W, k, rows[0], rows[1], 2), (k, rows)
                total, parts = r.last_kernel_ms(), r.last_launch_parts()
                assert sum(n for _, n in parts) == 2 * (rows[1] - rows[0]) * W
                print(f"{precision} k {k} rows {rows}: {total:.3f} ms = producer {ms_coarse:.3f} ms over {rays_coarse} rays + consumer {parts}")
                slack = 1e-3          # HIP event differences are rounded to the microsecond
                assert ms_coarse > 0 and all(ms > 0 for ms, _ in parts)
                assert total >= ms_coarse and total + slack >= ms_coarse + sum(ms for ms, _ in parts)
        finally:
            r.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------

def test_every_other_call_is_refused_by_name_and_leaves_the_last_launch_alone():
    H, W = 7, 19
    r, fresh = _renderer(k=2), _renderer()
    try:
        good = _frame(r, H, W)
        state = lambda: (r.last_kernel_ms(), r.last_launch_parts(), r.last_ray_evaluations(), r.last_coarse_launch())
        before = state()
        rays = fresh.create_rays(_poses(1), H, W, **_camera(H, W))

        def refused(call, match="shared_coarse"):
            with pytest.raises(NotImplementedError, match=match):
                call()
            assert state() == before

        for extra in ("disp", "z_std", "rgb_coarse", "depth_coarse", "acc_coarse", "raw_fine", "raw_coarse", "z_fine", "weights_coarse",
                      "sample_cond"):
            for precision in ("f16x3", "f32"):
                refused(lambda: _frame(r, H, W, precision=precision, outputs=LEAN + (extra,)))
        refused(lambda: _frame(r, H, W, precision="f32", outputs=LEAN + ("feat_map",)))
        for precision in ("f16x3", "f16x1", "f32"):
            refused(lambda: r.render_rays(rays, precision=precision))
        refused(lambda: r.render_rays(rays, debug_fine_depths=torch.zeros(len(rays), 192)))
        refused(lambda: r.render_rays(rays, debug_coarse_weights=torch.zeros(len(rays), 64)))
        # the refusals that exist without it come first and keep their text
        refused(lambda: _frame(r, H, W, outputs=LEAN + ("feat_map",)), match="feat_map .* NWE_PREC_F32 kernel only")
        # together with early termination every call is refused, and the message names both settings
        r.set_early_termination(1e-2)
        for precision in ("f16x3", "f32"):
            refused(lambda: _frame(r, H, W, precision=precision), match="shared_coarse.*early termination")
        refused(lambda: r.render_rays(rays), match="shared_coarse.*early termination")
        r.set_early_termination(0.0)
        # the next legal render is unaffected (and no hook stayed armed)
        _same(_frame(r, H, W), good, "after the refusals")
        r.set_shared_coarse(1)
        _same(r.render_rays(rays, outputs=LEAN + ("z_fine",)), fresh.render_rays(rays, outputs=LEAN + ("z_fine",)), "render_rays, k back to 1")
    finally:
        r.close(); fresh.close()


def test_unfolded_networks_are_refused_under_the_mfma_precisions():
    """nwe_debug_set_fold(0) packs the reference formulation, a comparison path that has no sharing kernel: refused by name
    under f16x3 / f16x1, rendered by the fp32 kernel - the bits of the fp32 kernel on folded networks, which reads the same
    fp32 weights - and rendered again once k is back to 1."""
    H, W = 7, 19
    r, folded = _renderer(fold=False), _renderer(k=2)
    try:
        plain = _frame(r, H, W)
        ms = r.last_kernel_ms()
        r.set_shared_coarse(2)
        for precision in ("f16x3", "f16x1"):
            with pytest.raises(NotImplementedError, match=r"shared_coarse.*nwe_debug_set_fold\(0\)"):
                _frame(r, H, W, precision=precision)
            assert r.last_kernel_ms() == ms
        _same(_frame(r, H, W, precision="f32"), _frame(folded, H, W, precision="f32"), "unfolded f32")
        r.set_shared_coarse(1)
        _same(_frame(r, H, W), plain, "unfolded, k back to 1")
    finally:
        r.close(); folded.close()


# ---- 7. a long-lived context --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_switching_k_across_frames_equals_fresh_contexts(precision):
    """k 1 -> 4 -> 2 -> 1 over frames of 7 x 19, 64 x 64 and 7 x 19 again: the weight tables of the launch slots grow and are
    reused (more frames than slots), and every frame is the one a fresh context renders."""
    r = _renderer()
    try:
        for k in (1, 4, 2, 1):
            r.set_shared_coarse(k)
            for H, W in ((7, 19), (64, 64), (7, 19)):
                got = _frame(r, H, W, precision=precision)
                counts = (r.last_ray_evaluations(), (r.last_coarse_launch() or (0, 0))[1])
                fresh = _renderer(k=k)
                try:
                    _same(got, _frame(fresh, H, W, precision=precision), (precision, k, H, W))
                    assert counts == (SC.evaluations(H, W, k, 0, H, 1, 64, 128), SC.n_rep(H, W, k, 0, H, 1) if k > 1 else 0)
                finally:
                    fresh.close()
    finally:
        r.close()


def test_frames_queued_on_two_streams_equal_the_sequential_ones():
    """Two shared frames of different poses and k in flight on two streams without a synchronisation between them: each launch
    owns its weight table."""
    H, W = 64, 64
    r = _renderer()
    try:
        jobs = [(4, _poses(2)[0]), (2, _poses(2)[1]), (4, _poses(2)[1]), (2, _poses(2)[0])]
        want = []
        for k, pose in jobs:
            r.set_shared_coarse(k)
            want.append({key: v.clone() for key, v in _frame(r, H, W, poses=pose).items()})
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in range(2)]
        got = []
        for i, (k, pose) in enumerate(jobs):
            r.set_shared_coarse(k)
            with torch.cuda.stream(streams[i % 2]):
                got.append(_frame(r, H, W, poses=pose))
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            _same(a, b, ("stream job", i))
    finally:
        r.close()


def test_set_sampling_behind_a_shared_frame_in_flight_leaves_it_unchanged():
    """nwe_set_sampling waits for the launches of the context, the producer and the consumer of the frame included, before it
    rewrites the tables they read; the setting itself is copied at launch."""
    H, W = 200, 300
    r = _renderer(k=4)
    try:
        want = {key: v.clone() for key, v in _frame(r, H, W).items()}
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = _frame(r, H, W)
        r.set_sampling(24, 40)
        r.set_shared_coarse(1)
        torch.cuda.synchronize()
        _same(got, want, "frame in flight")
        after = _frame(r, H, W)
        fresh = _renderer(ns=24, ni=40)
        try:
            _same(after, _frame(fresh, H, W), "after set_sampling")
        finally:
            fresh.close()
    finally:
        r.close()


def test_handler_applies_the_setting_and_raises_what_the_abi_says(monkeypatch):
    sd_c, sd_f = _nets("8x256")
    monkeypatch.setenv("NWE_SHARED_COARSE", "4")
    h = nwe_amd.NeRFReplicaInferenceHandler("office_geneve", "unused.ckpt")
    h.set_sampling(64, 128)
    h.initialize_models((sd_c, sd_f))
    try:
        assert h.renderer.shared_coarse == 4
        out = h.render(_poses(1)[0], 7, 19)
        assert h.renderer.last_ray_evaluations() == SC.evaluations(7, 19, 4, 0, 7, 1, 64, 128) and torch.isfinite(out["rgb"]).all()
        rays = h.renderer.create_rays(_poses(1), 7, 19, **_camera(7, 19))
        with pytest.raises(NotImplementedError, match="shared_coarse"):
            h._render_rays(rays)
    finally:
        h.renderer.close()
