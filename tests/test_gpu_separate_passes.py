"""Separate passes on the GPU (include/nwe.h: nwe_set_separate_passes): the coarse and the fine pass of a call as two launches,
each with the kernels of its own network's shape.

The mode is exact, so nothing here has a tolerance but the comparisons with the oracle: with two networks of one shape every
output equals the fused call's bit for bit; with two shapes the coarse outputs are those of a (coarse, coarse) context and the
rest those of a (fine, fine) context fed these coarse weights - calls that exist without the mode.  Frames are a few hundred
rays: 7 x 19 with two poses (266 rays: a ragged last packet, odd in both directions) and 12 x 64.
"""
import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import synthetic
from oracle import nerf_oracle as O
from tests import early_termination as E
from tests import mode_domain as M
from tests import shape_domain as S
from tests import shared_coarse as SC

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4                                    # tests/test_gpu_parity.py
LEAN = ("rgb", "depth", "acc")
COARSE = ("rgb_coarse", "depth_coarse", "acc_coarse", "disp_coarse", "raw_coarse", "weights_coarse")
REST = ("rgb", "depth", "acc", "disp", "z_std", "raw_fine", "z_fine", "sample_cond", "sample_amp", "sample_switch")
FULL = REST + COARSE
FRAMES = {"7x19x2": (7, 19, 2), "12x64": (12, 64, 1)}
# name -> (depth, width, view directions): "4x128", "8x256", "4x128-noview", "8x256-noview" and every other shape with MFMA kernels
NETS = M.NETS


def _sd(kind, seed):
    D, W, view = NETS[kind]
    return synthetic.make_state_dict(seed, D, W, use_view_dirs=view)


def _renderer(coarse, fine, ns=64, ni=128, on=False, devices=None, white=False):
    """Network `coarse` with seed 1000 in slot 0, `fine` with seed 1001 in slot 1: a network is the same in every context."""
    r = nwe_amd.TiledRenderer(devices) if devices else nwe_amd.Renderer(0)
    r.set_network(0, _sd(coarse[0], coarse[1]) if isinstance(coarse, tuple) else _sd(coarse, 1000))
    r.set_network(1, _sd(fine[0], fine[1]) if isinstance(fine, tuple) else _sd(fine, 1001))
    r.set_sampling(ns, ni)
    r.set_white_background(white)
    r.set_separate_passes(on)
    return r


def _camera(H, W):
    fx, fy, cx, cy = O.intrinsics(H, W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=E.NEAR, far=E.FAR)


def _poses(n_poses):
    return E.frame_rays(1, 1, n_poses)[0].numpy()


def _frame(r, H, W, n_poses=1, precision="f16x3", rows=None, outputs=LEAN, poses=None):
    return r.render(_poses(n_poses) if poses is None else poses, H, W, rows=rows, precision=precision, outputs=outputs, **_camera(H, W))


def _same(a, b, ctx, keys=None):
    keys = [k for k in a if not k.startswith("_") and k != "flags"] if keys is None else keys
    for key in keys:
        assert torch.equal(torch.nan_to_num(a[key], nan=-7.0), torch.nan_to_num(b[key], nan=-7.0)), (ctx, key)
    assert int(a["flags"].item()) == int(b["flags"].item()), (ctx, hex(int(a["flags"].item())), hex(int(b["flags"].item())))


def _train_tables(R, ns, ni, seed=5):
    g = torch.Generator().manual_seed(seed)
    return {"t_rand": torch.rand(R, ns, generator=g), "noise_coarse": 0.3 * torch.randn(R, ns, generator=g),
            "noise_fine": 0.3 * torch.randn(R, ns + ni, generator=g), "u": torch.rand(R, ni, generator=g)}


CASES = [
    ("4x128", 64, 128, "f16x3", False),
    ("8x256", 64, 128, "f16x3", True),
    ("4x128-noview", 64, 128, "f16x1", False),
    ("4x128", 7, 6, "f16x1", True),
    ("8x256", 7, 6, "f16x3", False),
    ("4x128", 96, 32, "f16x3", True),          # more than 64 coarse samples: both launches are sample-split
    ("4x128-noview", 96, 32, "f16x1", False),
]


# ---- 1. one shape: the fused call, bit for bit --------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,ns,ni,precision,white", CASES)
def test_same_shape_equals_the_fused_call_bit_for_bit(kind, ns, ni, precision, white):
    """Every call kind with the mode off and on, on one context: lean frames under the three forced plans, frames with every
    output, render_rays with every output, with training tables on host-drawn random numbers, with given fine depths and with
    given raw outputs.  torch.equal on every output and equal flag words."""
    view = NETS[kind][2]
    r = _renderer(kind, kind, ns, ni, white=white)
    plans = (1,) if ns > 64 else (0, 1, 2)
    try:
        rays = S.frame_rays(view).cuda()
        R = rays.shape[0]
        train = _train_tables(R, ns, ni)
        g = torch.Generator().manual_seed(9)
        raw = (torch.randn(R, ns, 4, generator=g), torch.randn(R, ns + ni, 4, generator=g))

        def calls():
            out = {}
            for name, (H, W, n_poses) in FRAMES.items():
                out["lean", name] = _frame(r, H, W, n_poses, precision)
                out["full", name] = _frame(r, H, W, n_poses, precision, outputs=FULL)
            out["rows"] = _frame(r, 7, 19, 2, precision, rows=(3, 6), outputs=LEAN + ("rgb_coarse", "z_fine"))
            out["rays"] = r.render_rays(rays, precision=precision, outputs=FULL)
            out["rays-lean"] = r.render_rays(rays, precision=precision, outputs=LEAN)
            out["train"] = r.render_rays(rays, precision=precision, outputs=FULL, train=train)
            out["depths"] = r.render_rays(rays, precision=precision, outputs=FULL, debug_fine_depths=out["rays"]["z_fine"])
            out["raw"] = r.render_rays(rays, precision=precision, outputs=FULL, debug_raw=raw)
            out["raw-coarse"] = r.render_rays(rays, precision=precision, outputs=FULL, debug_raw=(raw[0], None))
            return out

        off = calls()
        assert r.last_coarse_launch() is None
        r.set_separate_passes(True)
        for plan in plans + (-1,):
            r.debug_set_decomposition(plan)
            on = calls()
            assert r.last_coarse_launch()[1] == R
            for key in off:
                _same(on[key], off[key], (kind, ns, ni, precision, white, plan, key))
        r.debug_set_decomposition(-1)
        # the coarse-weights hook: no coarse launch, the coarse outputs stay unwritten as without the mode
        w = off["rays"]["weights_coarse"]
        got = r.render_rays(rays, precision=precision, outputs=REST, debug_coarse_weights=w)
        assert r.last_coarse_launch() is None
        r.set_separate_passes(False)
        _same(got, r.render_rays(rays, precision=precision, outputs=REST, debug_coarse_weights=w), (kind, "coarse weights"))
        # ... and on the call's own weights its outputs are the call's; the coarse flag bits belong to the coarse pass it skips
        _same(got, dict(off["rays"], flags=off["rays"]["flags"] & 0x30F), (kind, "coarse weights vs the call itself"), REST)
    finally:
        r.close()


# ---- 2. two shapes: each pass is the pass of a one-shape context, bit for bit -------------------------------------------------

MIXED = [
    ("4x128", "8x256", 64, 128, "f16x3", False),
    ("8x256", "4x128", 64, 128, "f16x3", True),
    ("4x128", "8x256", 7, 6, "f16x1", True),
    ("8x256", "4x128", 96, 32, "f16x1", False),
    ("4x128", "8x256", 96, 32, "f16x3", False),
    ("4x128-noview", "8x256-noview", 64, 128, "f16x3", True),
]


def _expected_mixed(coarse, fine, ns, ni, precision, white, rays):
    """Context A holds (coarse, coarse): its coarse outputs and weights.  Context B holds (fine, fine): everything else, on A's
    weights through the coarse-weights hook.  Both render with the fused kernels."""
    return M.expected_mixed(lambda c, f: _renderer(c, f, ns, ni, white=white), coarse, fine, precision, rays, COARSE, REST)


@pytest.mark.parametrize("coarse,fine,ns,ni,precision,white", MIXED)
def test_mixed_shapes_equal_the_passes_of_one_shape_contexts(coarse, fine, ns, ni, precision, white):
    """render_rays and render of the same pixels (7 x 19, two poses) on a (coarse, fine) context with the mode on: the coarse
    outputs are context A's and the others context B's, bit for bit; the flag word is the fp32 kernel's for the same pair."""
    H, W, n_poses = FRAMES["7x19x2"]
    view = NETS[coarse][2]
    M = _renderer(coarse, fine, ns, ni, on=True, white=white)
    try:
        rays = M.create_rays(_poses(n_poses), H, W, use_view_dirs=view, **_camera(H, W))
        a, b = _expected_mixed(coarse, fine, ns, ni, precision, white, rays)
        flags = M.render_rays(rays, precision="f32", outputs=FULL)["flags"]
        want = dict(a, **b)
        want["flags"] = flags
        for plan in ((1,) if ns > 64 else (0, 1, 2)):
            M.debug_set_decomposition(plan)
            _same(M.render_rays(rays, precision=precision, outputs=FULL), want, (coarse, fine, ns, ni, precision, plan, "render_rays"), FULL)
            _same(_frame(M, H, W, n_poses, precision, outputs=FULL), want, (coarse, fine, ns, ni, precision, plan, "render"), FULL)
            _same(_frame(M, H, W, n_poses, precision), want, (coarse, fine, ns, ni, precision, plan, "lean render"), LEAN)
            _same(M.render_rays(rays, precision=precision, outputs=REST), want, (coarse, fine, ns, ni, precision, plan, "no coarse output"), REST)
    finally:
        M.close()


# ---- 3. two shapes against the references -------------------------------------------------------------------------------------

def test_mixed_shapes_against_the_oracle_and_the_fp32_kernel():
    """c4x128-f8x256 of tests/shape_domain.py at the YAML's 64 + 128: within RGB_TOL of the live oracle and of the fp32 kernel
    off the oracle's own cliff rays (the mask and the cap of test_handler_renders_two_mfma_shapes_that_differ_with_f32)."""
    b = S.build(S.BY_NAME["c4x128-f8x256"])
    ref = O.render_rays(b.rays, S.tensors(b.sd_c), S.tensors(b.sd_f), O.RenderConfig())
    ok = ref["raw_fine"][:, -1, 3].abs().numpy() > 1e-5
    r = nwe_amd.Renderer(0)
    try:
        r.set_network(0, b.sd_c); r.set_network(1, b.sd_f)
        r.set_sampling(64, 128)
        r.set_separate_passes(True)
        got = r.render_rays(b.rays.cuda(), precision="f16x3", outputs=LEAN + ("rgb_coarse",))
        f32 = r.render_rays(b.rays.cuda(), precision="f32", outputs=LEAN + ("rgb_coarse",))
        e_ref = np.abs(got["rgb"].cpu().numpy() - ref["rgb_fine"].numpy())[ok].max()
        e_f32 = np.abs(got["rgb"].cpu().numpy() - f32["rgb"].cpu().numpy())[ok].max()
        e_c = np.abs(got["rgb_coarse"].cpu().numpy() - ref["rgb_coarse"].numpy()).max()
        print(f"c4x128-f8x256 f16x3 separate passes: max|rgb - oracle| {e_ref:.2e}, vs fp32 kernel {e_f32:.2e}, coarse vs oracle {e_c:.2e}, "
              f"kept {ok.mean():.3f}")
        assert ok.mean() >= 0.95
        assert e_ref <= RGB_TOL and e_f32 <= RGB_TOL and e_c <= RGB_TOL
    finally:
        r.close()


# ---- 4. with the shared coarse pass -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("coarse,fine,ns,ni,precision,white", MIXED[:4])
def test_shared_coarse_pass_composes_with_a_mixed_pair(k, coarse, fine, ns, ni, precision, white):
    """The expectation of tests/test_gpu_shared_coarse.py with the passes taken from the one-shape contexts: Z = z_fine of
    context B on context A's weights, then every ray's fine pass in B on Z[rep]."""
    H, W, n_poses = FRAMES["7x19x2"]
    M = _renderer(coarse, fine, ns, ni, on=True, white=white)
    B = _renderer((fine, 1001), fine, ns, ni, white=white)
    try:
        rays = M.create_rays(_poses(n_poses), H, W, **_camera(H, W))
        _, b = _expected_mixed(coarse, fine, ns, ni, precision, white, rays)
        rep = torch.from_numpy(SC.rep_index(H, W, k, 0, H, n_poses)).to(rays.device)
        want = B.render_rays(rays, precision=precision, outputs=LEAN, debug_fine_depths=b["z_fine"][rep].contiguous())
        M.set_shared_coarse(k)
        for plan in ((1,) if ns > 64 else (0, 1)):
            M.debug_set_decomposition(plan)
            got = _frame(M, H, W, n_poses, precision)
            _same(got, dict(want, flags=want["flags"] & 0x30F), (k, coarse, fine, ns, ni, precision, plan), LEAN)
            assert M.last_coarse_launch()[1] == SC.n_rep(H, W, k, 0, H, n_poses)
            assert M.last_ray_evaluations() == SC.evaluations(H, W, k, 0, H, n_poses, ns, ni)
    finally:
        M.close(); B.close()


# ---- 5. invariances -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f16x1"])
def test_row_tiles_pose_batches_context_tiles_and_plans_equal_the_frame(precision):
    H, W = 7, 19
    r = _renderer("4x128", "8x256", on=True)
    tiled = _renderer("4x128", "8x256", on=True, devices=[0, 0, 0])
    try:
        whole = _frame(r, H, W, 2, precision)
        parts = [_frame(r, H, W, 2, precision, rows=rows) for rows in ((0, 3), (3, 6), (6, 7))]
        for key in LEAN:
            w = whole[key].reshape((2, H, W) + tuple(whole[key].shape[1:]))
            rows = torch.cat([p[key].reshape((2, -1, W) + tuple(p[key].shape[1:])) for p in parts], 1)
            assert torch.equal(w, rows), (precision, key, "row tiles")
        for p in range(2):
            one = _frame(r, H, W, precision=precision, poses=_poses(2)[p])
            for key in LEAN:
                assert torch.equal(one[key], whole[key][p * H * W:(p + 1) * H * W]), (precision, key, "pose", p)
        out = _frame(tiled, H, W, 2, precision)
        assert tiled.last_tiled and all(p.separate_passes for p in tiled.parts)
        assert all(p.last_coarse_launch() is not None for p in tiled.parts)
        _same(out, whole, (precision, "context tiles"), LEAN)
        # 200 x 300: one full round of packet workgroups and a sample-split rest under the hybrid plan
        for Hp, Wp in ((H, W), (200, 300)):
            res = {}
            for plan in (0, 1, 2):
                r.debug_set_decomposition(plan)
                res[plan] = _frame(r, Hp, Wp, precision=precision)
                assert r.debug_last_plan() == plan
            r.debug_set_decomposition(-1)
            for other in (res[1], res[2], _frame(r, Hp, Wp, precision=precision)):
                _same(res[0], other, (precision, Hp, Wp, "plans"), LEAN)
    finally:
        r.close(); tiled.close()


# ---- 6. introspection ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("outputs", [LEAN, LEAN + ("rgb_coarse",)])
def test_introspection_after_a_mixed_frame(outputs):
    H, W = 12, 64
    r = _renderer("4x128", "8x256", on=True)
    try:
        _frame(r, H, W, outputs=outputs)
        ms_coarse, rays_coarse = r.last_coarse_launch()
        total, parts = r.last_kernel_ms(), r.last_launch_parts()
        print(f"{outputs}: {total:.3f} ms = coarse {ms_coarse:.3f} ms over {rays_coarse} rays + fine {parts}")
        assert rays_coarse == H * W and sum(n for _, n in parts) == H * W
        assert r.last_ray_evaluations() == (H * W * 256,) * 2
        assert ms_coarse > 0 and all(ms > 0 for ms, _ in parts)
        assert total >= ms_coarse and total + 1e-3 >= ms_coarse + sum(ms for ms, _ in parts)   # events are rounded to the microsecond
        # without importance samples there is one pass and one launch
        r.set_sampling(32, 0)
        _frame(r, H, W, outputs=LEAN)
        assert r.last_coarse_launch() is None and r.last_ray_evaluations() == (H * W * 32,) * 2
    finally:
        r.close()


# ---- 7. refusals and state ----------------------------------------------------------------------------------------------------

def test_refusals_by_name_leave_the_context_as_it_was():
    H, W = 7, 19
    r = _renderer("4x128", "8x256", on=True)
    try:
        good = _frame(r, H, W)
        state = lambda: (r.last_kernel_ms(), r.last_launch_parts(), r.last_ray_evaluations(), r.last_coarse_launch())
        before = state()
        rays = r.create_rays(_poses(1), H, W, **_camera(H, W))
        r.set_early_termination(1e-2)
        for precision in ("f16x3", "f16x1"):
            for _ in range(3):                               # more refusals than a ring of four slots would forgive
                with pytest.raises(NotImplementedError, match="separate passes.*early termination"):
                    _frame(r, H, W, precision=precision)
                assert state() == before
        # the refusals early termination has on its own come first and keep their text
        with pytest.raises(NotImplementedError, match="early termination is on.*nwe_render_rays"):
            r.render_rays(rays)
        assert state() == before
        r.set_early_termination(0.0)
        # a pair with and without view directions: the refusal that exists without the mode, by name
        r.set_network(1, _sd("8x256-noview", 1001))
        with pytest.raises(RuntimeError, match="both have, or both lack, view directions"):
            _frame(r, H, W)
        assert state() == before
        r.set_network(1, _sd("8x256", 1001))
        # one network packed unfolded, the other folded
        r.debug_set_fold(False)
        r.set_network(1, _sd("8x256", 1001))
        with pytest.raises(NotImplementedError, match="separate passes.*same formulation"):
            _frame(r, H, W)
        assert state() == before
        r.debug_set_fold(True)
        r.set_network(1, _sd("8x256", 1001))
        _same(_frame(r, H, W), good, "after the refusals")
        # off again: the pair is refused as it always was
        r.set_separate_passes(False)
        with pytest.raises(NotImplementedError, match="same shape"):
            _frame(r, H, W)
    finally:
        r.close()


def test_unfolded_networks_render_through_the_full_kernels():
    """nwe_debug_set_fold(0) has no sharing kernels: a lean frame then takes the full kernels' two launches, the fused call's bits."""
    H, W = 7, 19
    r = nwe_amd.Renderer(0)
    try:
        r.debug_set_fold(False)
        r.set_network(0, _sd("4x128", 1000)); r.set_network(1, _sd("4x128", 1001))
        r.set_sampling(64, 128)
        off = _frame(r, H, W, 2)
        r.set_separate_passes(True)
        _same(_frame(r, H, W, 2), off, "unfolded")
        assert r.last_coarse_launch()[1] == 2 * H * W
    finally:
        r.close()


def test_toggling_on_a_long_lived_context_equals_fresh_contexts():
    """off -> on -> off -> on over frames of growing and shrinking size (the slots' tables grow and are reused: more frames
    than slots), lean and with coarse outputs."""
    r = _renderer("8x256", "8x256")
    fresh = {on: _renderer("8x256", "8x256", on=on) for on in (False, True)}
    outs = LEAN + ("rgb_coarse", "weights_coarse")
    try:
        for on in (False, True, False, True):
            r.set_separate_passes(on)
            assert r.separate_passes is on
            for H, W in ((7, 19), (64, 64), (7, 19)):
                _same(_frame(r, H, W), _frame(fresh[on], H, W), (on, H, W, "lean"))
                counts = (r.last_ray_evaluations(), r.last_coarse_launch() is not None)
                assert counts == ((H * W * 256,) * 2, on)
                _same(_frame(r, H, W, outputs=outs), _frame(fresh[on], H, W, outputs=outs), (on, H, W, "coarse outputs"))
    finally:
        r.close()
        for f in fresh.values():
            f.close()


@pytest.mark.parametrize("outputs", [LEAN, LEAN + ("depth_coarse",)])
def test_six_launches_on_six_streams_equal_the_serial_ones(outputs):
    """More launches in flight than the ring has slots, on six streams without a synchronisation between them: every launch
    owns its weight table."""
    H, W = 64, 64
    r = _renderer("4x128", "8x256", on=True)
    try:
        poses = E.frame_rays(1, 1, 6)[0].numpy()
        want = [{k: v.clone() for k, v in _frame(r, H, W, poses=poses[i], outputs=outputs).items()} for i in range(6)]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in range(6)]
        got = []
        for i in range(6):
            with torch.cuda.stream(streams[i]):
                got.append(_frame(r, H, W, poses=poses[i], outputs=outputs))
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            _same(a, b, ("stream job", i))
    finally:
        r.close()


# ---- 8. handler ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["argument", "environment"])
def test_handler_keeps_two_mfma_shapes_on_the_mfma_path(how, monkeypatch, capsys):
    b = S.build(S.BY_NAME["c4x128-f8x256"])
    if how == "environment":
        monkeypatch.setenv("NWE_SEPARATE_PASSES", "1")
        h = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "unused")
    else:
        h = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "unused", separate_passes=True)
    h.initialize_models(state_dicts=(b.sd_c, b.sd_f))
    try:
        said = capsys.readouterr().out
        assert h._precision == "f16x3" and h.renderer.separate_passes and said == ""
        pose = O.camera_pose((0.0, -0.5, -0.76, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))
        got = h.render(pose[0].numpy(), S.FRAME_H, S.FRAME_W)["rgb"].reshape(-1, 3).cpu().numpy()[:S.N_RAYS]
        assert h.renderer.last_coarse_launch()[1] == S.FRAME_H * S.FRAME_W
        ref = O.render_rays(b.rays, S.tensors(b.sd_c), S.tensors(b.sd_f), O.RenderConfig())           # the YAML's 64 + 128
        ok = ref["raw_fine"][:, -1, 3].abs().numpy() > 1e-5
        err = np.abs(got - ref["rgb_fine"].numpy())[ok].max()
        print(f"handler, {how}: max|rgb - oracle| {err:.2e}, kept {ok.mean():.3f}")
        assert ok.mean() >= 0.95 and err <= RGB_TOL
    finally:
        h.renderer.close()
