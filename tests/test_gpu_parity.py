"""Parity of the HIP render path (through the C ABI) against the CPU oracle and the committed goldens.

Tolerances (BASELINE.md §4 / north_star): float RGB max-abs <= 1e-4 per channel and PSNR > 50 dB; depth is
compared as max-abs / far (<= 1e-4) because its range is 0..10; rays whose last-sample raw sigma is within
1e-5 of zero are "cliff rays" (alpha_last = 1-exp(-relu(sigma)*1e10*|d|) is a step function of the sign,
nerf/models/model_utils.py:54) and are counted and bounded separately, never silently dropped.
"""
import os

import numpy as np
import pytest
import torch

import nwe_amd
from oracle import nerf_oracle as O
from tests import input_domain

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4
FAR = 10.0


def _sd(seed, D, W):
    return nwe_amd.synthetic.make_state_dict(seed, D, W)


def _t(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


@pytest.fixture(scope="module")
def r_c3():
    r = nwe_amd.Renderer(0)
    r.set_network(0, _sd(1000, 8, 256))
    r.set_network(1, _sd(1001, 8, 256))
    r.set_sampling(64, 128)
    yield r
    r.close()


@pytest.fixture(scope="module")
def r_c1():
    r = nwe_amd.Renderer(0)
    r.set_network(0, _sd(1000, 4, 128))
    r.set_sampling(32, 0)
    yield r
    r.close()


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return 99.0 if mse == 0 else -10.0 * np.log10(mse)


def test_selftest_hardware_assumptions(r_c1):
    rc, rep = r_c1.selftest()
    print("selftest report:", rep)
    assert rep[0] == 0, "v_mfma_f32_32x32x16_f16 lane maps differ from the assumed ones"
    assert rep[1] == 0, "accumulator-as-B-operand k permutation differs from hidden_col()"
    assert rep[3] == 0, "LDS-DMA lane order differs"
    assert rc == 0
    assert rep[4] < 100, f"octave_sincos error {rep[4]}e-9: the positional encoding must be fp32-rounding accurate in every band"
    assert rep[5] < 500, f"expf relative error {rep[5]}e-9"
    # the whole documented range (|x / 10| <= 5e4, lowest-octave arguments up to 1.6e6 rad): the reference's own sinf error
    # there plus one fp32 ulp (tests/test_input_domain_oracle.py derives the bound of tests/input_domain.py); beyond it NaN in every octave (-1 if not)
    assert 0 <= rep[7] < input_domain.SINCOS_WIDE_BOUND, f"octave_sincos over its documented range: {rep[7]}e-9 (-1: a finite value beyond it)"


def test_create_rays_bit_exact(r_c1, golden_dir):
    """nwe_create_rays against the reference's create_rays output (nerf/rays/rays.py:6-32), every bit."""
    g = np.load(os.path.join(golden_dir, "rays.npz"))
    for (H, W) in [(4, 6), (64, 64)]:
        fx, fy, cx, cy = O.intrinsics(H, W)
        for name in ("hor0", "hor30", "tilt"):
            got = r_c1.create_rays(g[f"pose_{name}"], H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0).cpu().numpy()
            gold = g[f"rays_{H}x{W}_{name}"]
            bad_cols = [c for c in range(11) if not np.array_equal(got[:, c], gold[:, c])]
            assert not bad_cols, (H, W, name, bad_cols, np.abs(got - gold).max(0))
    fx, fy, cx, cy = O.intrinsics(800, 800)
    for name in ("hor0", "hor30"):
        got = r_c1.create_rays(g[f"pose_{name}"], 800, 800, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0)
        got = got.reshape(800, 800, 11)[::37, ::37].cpu().numpy()
        assert np.array_equal(got, g[f"rays_800_stride37_{name}"]), name


def test_ray_generation_is_bit_exact(r_c1, golden_dir):
    """nwe_render (in-kernel rays from the pose) == nwe_render_rays on the reference's own rays, bit for bit,
    in the fp32 mode: only possible if origins, directions and view dirs are generated bit-exactly."""
    g = np.load(os.path.join(golden_dir, "rays.npz"))
    fx, fy, cx, cy = O.intrinsics(64, 64)
    for name in ("hor0", "hor30", "tilt"):
        rays = torch.from_numpy(g[f"rays_64x64_{name}"]).cuda()
        a = r_c1.render_rays(rays, precision="f32", outputs=("rgb", "depth", "acc", "raw_coarse"))
        b = r_c1.render(g[f"pose_{name}"], 64, 64, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, precision="f32",
                        outputs=("rgb", "depth", "acc", "raw_coarse"))
        for k in ("rgb", "depth", "acc", "raw_coarse"):
            assert torch.equal(a[k], b[k]), (name, k, (a[k] - b[k]).abs().max().item())


def test_ray_generation_800_subset(r_c1, golden_dir):
    g = np.load(os.path.join(golden_dir, "rays.npz"))
    fx, fy, cx, cy = O.intrinsics(800, 800)
    for name in ("hor0", "hor30"):
        gold = g[f"rays_800_stride37_{name}"]                     # [22, 22, 11] rows/cols 0, 37, 74, ...
        for ri, row in enumerate(range(0, 800, 37)):
            a = r_c1.render(g[f"pose_{name}"], 800, 800, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, rows=(row, row + 1),
                            precision="f32", outputs=("rgb", "raw_coarse"))
            b = r_c1.render_rays(torch.from_numpy(gold[ri]).cuda(), precision="f32", outputs=("rgb", "raw_coarse"))
            assert torch.equal(a["raw_coarse"][::37], b["raw_coarse"]), (name, row)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_c1_frame_against_golden(r_c1, golden_dir, precision):
    """BASELINE config 1: 64x64, 32 samples, coarse-only 4x128."""
    g = np.load(os.path.join(golden_dir, "e2e_c1.npz"))
    fx, fy, cx, cy = O.intrinsics(64, 64)
    out = r_c1.render(g["pose"], 64, 64, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, precision=precision,
                      outputs=("rgb", "depth", "acc", "disp", "rgb_coarse", "raw_coarse"))
    raw = out["raw_coarse"].cpu().numpy()
    print(precision, "raw max err", np.abs(raw[:256] - g["raw_coarse_first256"]).max())
    assert np.abs(raw[:256] - g["raw_coarse_first256"]).max() < 5e-5
    cliff = np.abs(raw[:, -1, 3]) < 1e-5
    rgb = out["rgb"].cpu().numpy()
    err = np.abs(rgb - g["rgb_coarse"])
    print(precision, "rgb max err", err[~cliff].max(), "cliff rays", int(cliff.sum()), "psnr", psnr(rgb, g["rgb_coarse"]))
    assert err[~cliff].max() <= RGB_TOL
    assert psnr(rgb, g["rgb_coarse"]) > 50
    assert np.abs(out["depth"].cpu().numpy() - g["depth_coarse"])[~cliff].max() / FAR <= 1e-4
    assert np.abs(out["acc"].cpu().numpy() - g["acc_coarse"])[~cliff].max() <= 1e-4
    assert torch.equal(out["rgb"], out["rgb_coarse"])     # coarse-only: the fine slots carry the coarse result
    assert int(out["flags"].item()) & 0x7 == 0
    d_ref, d = g["disp_coarse"], out["disp"].cpu().numpy()
    assert np.array_equal(np.isnan(d_ref), np.isnan(d)) or cliff.any()    # acc == 0 -> NaN, like torch.max


def sampler_first_order_bound(amp, dcdf):
    """|dz| a change `dcdf` of the coarse cdf can cause at first order: z = bin_lo + (u - cdf_lo) / denom * width
    (nerf/rays/rays.py:118-119) moves by width/denom * (|d cdf_lo| + t |d denom|) <= 3 * amp * dcdf (dcdf = the largest
    change of a cdf entry, so a step changes by at most twice that); the inverse cdf is continuous across bin edges, so the
    bound holds when a sample changes bins.  Measured: a third of it at most.  The 2e-6 floor leaves room for the fp32
    rounding of z itself (depths up to 10)."""
    return 3.0 * amp * dcdf + 2e-6


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("pose", ["hor0", "hor30"])
def test_c3_subset_against_golden(r_c3, golden_dir, precision, pose):
    """BASELINE config 3 (800x800, 64+128, 8x256, raw random networks) on the committed strided 4096-ray subset: a closed
    per-ray chain from the pose to the pixel.

    With unrelated random coarse/fine networks the reference's importance sampling is ill conditioned on most rays: an
    importance sample in a nearly empty coarse bin moves by bin_width/denom ~ 4e3 (up to 1.5e4) times a change of the coarse
    cdf, and two fp32 evaluations of the coarse MLP (torch's sgemm blocking vs. any other order) differ by ~5e-7 in the
    weights.  So a pixel-level comparison alone cannot say whether a deviating ray is a bug; the chain can:
      T1   coarse pass, every ray: rgb / depth / acc at full tolerance and the coarse WEIGHTS (raw2outputs' 4th return,
           model_utils.py:80, the sampler's input) within 2e-6 of the reference's;
      T2a  the sampler on its OWN inputs, every ray: the reference's sample_pdf + sort (rays.py:74-121, handler.py:243) run on
           the kernel's coarse weights gives the kernel's depths (<= 1e-6; the kernel adds the weights in torch.sum's order);
      T2b  depths against the reference's, every ray: explained by the first-order bound 3 * amp * |d cdf| + 2e-6 with the
           measured cdf difference, except rays with a sample next to the `denom < 1e-5` switch (rays.py:114), which are
           counted;
      T3   fine pass ALONE, every ray, full tolerance, both directions: the oracle's fine pass on the kernel's depths, and
           the kernel's fine pass on the reference's depths (debug hook);
      T4   end to end: every ray whose depths agree (<= 2e-5) is within 1e-4; every other ray was explained in T2b and is
           counted; PSNR over all rays.
    """
    g = np.load(os.path.join(golden_dir, "e2e_c3_subset.npz"))
    fx, fy, cx, cy = O.intrinsics(800, 800)
    full = O.create_rays(torch.from_numpy(g[f"pose_{pose}"])[None], 800, 800, fx, fy, cx, cy, 0.1, 10.0)[0]
    rays_cpu = full[torch.from_numpy(g[f"idx_{pose}"])].contiguous()
    rays = rays_cpu.cuda()
    out = r_c3.render_rays(rays, precision=precision,
                           outputs=("rgb", "depth", "acc", "disp", "z_std", "rgb_coarse", "depth_coarse", "acc_coarse",
                                    "z_fine", "weights_coarse", "sample_cond", "sample_amp", "sample_switch"))
    tag = f"[{precision} {pose}]"
    # T1 ------------------------------------------------------------------------------------------
    cliff_c = np.abs(g[f"sigma_last_coarse_{pose}"]) < 1e-5
    errc = np.abs(out["rgb_coarse"].cpu().numpy() - g[f"rgb_coarse_{pose}"])
    w_k, w_ref = out["weights_coarse"].cpu(), torch.from_numpy(g[f"weights_coarse_{pose}"])
    werr = (w_k - w_ref).abs().numpy()
    werr[cliff_c, -1] = 0                       # the last weight of a cliff ray is the step function itself
    print(tag, "T1 coarse rgb max err", errc[~cliff_c].max(), "weights max err", werr.max(), "cliff rays", int(cliff_c.sum()))
    assert errc[~cliff_c].max() <= RGB_TOL
    assert np.abs(out["depth_coarse"].cpu().numpy() - g[f"depth_coarse_{pose}"])[~cliff_c].max() / FAR <= 1e-4
    assert np.abs(out["acc_coarse"].cpu().numpy() - g[f"acc_coarse_{pose}"])[~cliff_c].max() <= 1e-4
    assert werr.max() <= 2e-6
    # T2a -----------------------------------------------------------------------------------------
    z = out["z_fine"].cpu()
    t = torch.linspace(0., 1., 64)
    z_c = (rays_cpu[:, 6:7] * (1. - t) + rays_cpu[:, 7:8] * t)                                   # handler.py:216-218
    z_mid = .5 * (z_c[..., 1:] + z_c[..., :-1])                                                 # :236
    own = torch.sort(torch.cat([z_c, O.sample_pdf(z_mid, w_k[..., 1:-1], 128)], -1), -1).values  # :237-243 on the kernel's weights
    e2a = (own - z).abs().max(-1).values.numpy()
    print(tag, "T2a sampler on its own weights: max", e2a.max(), "rays > 1e-6:", int((e2a > 1e-6).sum()))
    assert e2a.max() <= 1e-6
    assert np.all(np.diff(z.numpy(), axis=1) >= 0)                                              # merge output is sorted
    dg_own = O.sample_pdf_diagnostics(z_mid, w_k[..., 1:-1], 128)
    for key, name, rel in (("min_denom", "sample_cond", 1e-5), ("amp", "sample_amp", 1e-3)):
        a_, b_ = out[name].cpu().numpy(), dg_own[key].numpy()
        assert np.max(np.abs(a_ - b_) / np.abs(b_)) <= rel, (name, np.max(np.abs(a_ - b_) / np.abs(b_)))
    assert np.max(np.abs(out["sample_switch"].cpu().numpy() - dg_own["switch"].numpy())) <= 1e-9
    # T2b -----------------------------------------------------------------------------------------
    z_ref = torch.sort(torch.cat([z_c, torch.from_numpy(g[f"z_samples_{pose}"])], -1), -1).values
    assert np.array_equal(z_ref[:64].numpy(), g[f"z_fine_first64_{pose}"])                      # the committed slice of the reference's own sort
    dz = (z - z_ref).abs().max(-1).values.numpy()
    dg_ref = O.sample_pdf_diagnostics(z_mid, w_ref[..., 1:-1], 128)
    dcdf = (dg_own["cdf"] - dg_ref["cdf"]).abs().max(-1).values.numpy()
    amp = np.maximum(dg_own["amp"].numpy(), dg_ref["amp"].numpy())
    near_switch = np.minimum(dg_own["switch"].numpy(), dg_ref["switch"].numpy()) <= 2.0 * dcdf  # a denom can land on either side of 1e-5
    bound = sampler_first_order_bound(amp, dcdf)
    unexplained = (dz > bound) & ~near_switch
    print(tag, f"T2b depths vs reference: {int((dz > 2e-5).sum())} rays differ by > 2e-5 (max {dz.max():.2e}); cdf difference median "
          f"{np.median(dcdf):.1e} max {dcdf.max():.1e}; amplification median {np.median(amp):.0f} max {amp.max():.0f}; "
          f"max dz/bound {np.max(dz / bound):.2f}; switch-adjacent rays {int(near_switch.sum())}; unexplained {int(unexplained.sum())}")
    assert not unexplained.any()
    assert near_switch.sum() <= 2                                                        # measured: 0
    # T3 ------------------------------------------------------------------------------------------
    sf = _t(_sd(1001, 8, 256))
    fo = O.fine_pass_given_depths(rays_cpu, z, sf, O.RenderConfig())
    cliff = fo["raw_fine"][:, -1, 3].abs().numpy() < 1e-5
    e3 = np.abs(out["rgb"].cpu().numpy() - fo["rgb_fine"].numpy())
    print(tag, "T3 fine pass on the kernel's depths: rgb max err", e3[~cliff].max(), "depth", np.abs(out["depth"].cpu().numpy() - fo["depth_fine"].numpy())[~cliff].max(),
          "cliff rays", int(cliff.sum()))
    assert e3[~cliff].max() <= RGB_TOL
    assert np.abs(out["depth"].cpu().numpy() - fo["depth_fine"].numpy())[~cliff].max() / FAR <= 1e-4
    assert np.abs(out["acc"].cpu().numpy() - fo["acc_fine"].numpy())[~cliff].max() <= 1e-4
    hook = r_c3.render_rays(rays[:64].contiguous(), precision=precision, outputs=("rgb", "depth", "raw_fine"),
                            debug_fine_depths=torch.from_numpy(g[f"z_fine_first64_{pose}"]))
    cl64 = np.abs(g[f"sigma_last_fine_{pose}"][:64]) < 1e-5
    eh = np.abs(hook["rgb"].cpu().numpy() - g[f"rgb_fine_{pose}"][:64])
    print(tag, "T3 kernel fine pass on the reference's depths: rgb max err", eh[~cl64].max(), "raw",
          np.abs(hook["raw_fine"].cpu().numpy() - g[f"raw_fine_first64_{pose}"]).max())
    assert eh[~cl64].max() <= RGB_TOL
    assert np.abs(hook["raw_fine"].cpu().numpy() - g[f"raw_fine_first64_{pose}"]).max() < 5e-5
    # T4 ------------------------------------------------------------------------------------------
    cliff_g = np.abs(g[f"sigma_last_fine_{pose}"]) < 1e-5
    rgb = out["rgb"].cpu().numpy()
    err = np.abs(rgb - g[f"rgb_fine_{pose}"]).max(-1)
    same_depths = (dz <= 2e-5) & ~cliff_g & ~cliff
    moved = err > RGB_TOL
    print(tag, f"T4 end to end: psnr {psnr(rgb, g[f'rgb_fine_{pose}']):.1f} dB, median {np.median(err):.1e}; rays with equal depths "
          f"{int(same_depths.sum())}, their max err {err[same_depths].max():.2e}; rays above 1e-4: {int(moved.sum())} "
          f"({moved.mean():.2%}), all with moved depths (min dz {dz[moved].min() if moved.any() else 0:.1e}), max {err.max():.1e}; "
          f"cliff rays {int(cliff_g.sum())}")
    assert err[same_depths].max() <= RGB_TOL                  # every ray sampled where the reference sampled it
    assert not (moved & (dz <= 2e-5) & ~cliff_g & ~cliff).any()   # a ray above tolerance has moved depths, explained in T2b
    assert psnr(rgb, g[f"rgb_fine_{pose}"]) > 50
    assert np.median(err) < 2e-6 and moved.mean() < 0.012 and err.max() < 1.5e-3      # measured: 0.46-0.71 % of the rays, max 6.1e-4
    assert cliff_g.sum() <= 8 and cliff_c.sum() <= 8


def _rays_at_points(pts, dirs):
    """Rays whose every sample sits exactly at `pts`: o = pts, near = far = 0 (z = 0*(1-t) + 0*t = 0, point = o + d*0 = o),
    view direction column = dirs as given (handler.py:210-214 takes it from the ray, it is not re-normalised)."""
    n = pts.shape[0]
    return torch.from_numpy(np.concatenate([pts, dirs, np.zeros((n, 2), np.float32), dirs], 1).astype(np.float32)).cuda()


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("tag,D,Wn,seed", [("4x128", 4, 128, 1000), ("8x256", 8, 256, 1001)])
def test_reference_mlp_vectors_through_the_kernels(golden_dir, precision, tag, D, Wn, seed):
    """tests/golden/mlp.npz (the reference's NeRFModel on 512 rows of [gamma(pts), gamma(dirs)], embed.npz's points incl.
    |x| ~ 20, -0.0, 1e-8: top-band arguments ~1000 rad) through the HIP kernels: Embedding + NeRFModel in isolation on
    reference-generated inputs (embedding.py:44-48, nerf_model.py:45-83).  Both decompositions of the MFMA kernel."""
    ge, gm = np.load(os.path.join(golden_dir, "embed.npz")), np.load(os.path.join(golden_dir, "mlp.npz"))
    x, y = gm[f"x_{tag}"], gm[f"y_{tag}"]
    enc = np.concatenate([ge["enc_xyz"], ge["enc_dir"]], 1)
    assert np.array_equal(x, np.concatenate([enc, enc], 0))          # the fixture's rows ARE gamma of embed.npz's points, twice
    rays = _rays_at_points(np.concatenate([ge["pts"]] * 2, 0), np.concatenate([ge["dirs"]] * 2, 0))
    assert float(np.abs(ge["pts"]).max()) > 15.0                      # the edge inputs are in there
    r = nwe_amd.Renderer(0)
    r.set_network(0, _sd(seed, D, Wn))
    r.set_sampling(2, 0)
    try:
        for mode in ((0, 1) if precision != "f32" else (-1,)):
            r.debug_set_decomposition(mode)
            raw = r.render_rays(rays, precision=precision, outputs=("raw_coarse",))["raw_coarse"].cpu().numpy()
            err = np.abs(raw - y[:, None, :])
            far_rows = np.abs(np.concatenate([ge["pts"]] * 2, 0)).max(-1) > 15.0
            print(f"[{precision} {tag} mode {mode}] raw vs reference NeRFModel: max {err.max():.2e}, on the |x| > 15 rows {err[far_rows].max():.2e}, "
                  f"|y| max {np.abs(y).max():.2f}")
            assert err.max() <= 5e-6
            assert np.array_equal(raw[:, 0], raw[:, 1])               # both samples sit at the same point
    finally:
        r.close()


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_reference_embedding_vectors_through_the_kernels(golden_dir, precision):
    """tests/golden/embed.npz through the kernels' positional encoding, component by component: a probe network carries ONE
    component of gamma(x) (or gamma(d)) unchanged to an output - layer 0 (resp. the view layer) selects it and adds 3 so that
    every ReLU is the identity, the other layers are identity matrices, the sigma (resp. red) head subtracts the 3 - and the
    output must be the reference's Embedding value (embedding.py:44-48) within 2e-6 at every point, |x| ~ 20 included."""
    ge = np.load(os.path.join(golden_dir, "embed.npz"))
    rays = _rays_at_points(ge["pts"], ge["dirs"])
    D, Wn = 4, 128
    shapes = nwe_amd.synthetic.layer_shapes(D, Wn, skips=())
    r = nwe_amd.Renderer(0)
    r.set_sampling(2, 0)
    worst = 0.0
    try:
        for comp in list(range(63)) + [63 + j for j in range(27)]:
            sd = {}
            for name, (n_out, n_in) in shapes.items():
                sd[name + ".weight"] = np.zeros((n_out, n_in), np.float32)
                sd[name + ".bias"] = np.zeros((n_out,), np.float32)
            for i in range(1, D):
                sd[f"_pts_linears.{i}.weight"][:] = np.eye(Wn, dtype=np.float32)
            sd["_feature_linear.weight"][:] = np.eye(Wn, dtype=np.float32)
            if comp < 63:           # gamma(x)[comp] -> h[0] -> sigma
                sd["_pts_linears.0.weight"][0, comp] = 1.0
                sd["_pts_linears.0.bias"][0] = 3.0
                sd["_alpha_linear.weight"][0, 0] = 1.0
                sd["_alpha_linear.bias"][0] = -3.0
                col = 3
            else:                   # gamma(d)[comp - 63] -> view layer output 0 -> red
                sd["_views_linears.0.weight"][0, Wn + comp - 63] = 1.0
                sd["_views_linears.0.bias"][0] = 3.0
                sd["_rgb_linear.weight"][0, 0] = 1.0
                sd["_rgb_linear.bias"][0] = -3.0
                col = 0
            r.set_network(0, sd)
            raw = r.render_rays(rays, precision=precision, outputs=("raw_coarse",))["raw_coarse"].cpu().numpy()[:, 0, col]
            want = ge["enc_xyz"][:, comp] if comp < 63 else ge["enc_dir"][:, comp - 63]
            e = float(np.abs(raw - want).max())
            worst = max(worst, e)
            assert e <= 2e-6, (comp, e)
    finally:
        r.close()
    print(f"[{precision}] gamma(x), gamma(d) of embed.npz through the kernel, all 90 components: max err {worst:.2e}")


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_fog_scene_every_ray_within_tolerance(golden_dir, precision):
    """Same geometry and fine network, thin-fog coarse network (synthetic.thin_fog): every coarse bin carries
    weight, the importance sampling is well conditioned, and the END-TO-END result must match the reference on
    EVERY ray: rgb 1e-4, depth/far 1e-4, acc 1e-4, z_std 1e-4, sample depths 2e-5."""
    g = np.load(os.path.join(golden_dir, "e2e_fog.npz"))
    r = nwe_amd.Renderer(0)
    r.set_network(0, nwe_amd.synthetic.thin_fog(_sd(1000, 8, 256)))
    r.set_network(1, _sd(1001, 8, 256))
    r.set_sampling(64, 128)
    fx, fy, cx, cy = O.intrinsics(800, 800)
    full = O.create_rays(torch.from_numpy(g["pose"])[None], 800, 800, fx, fy, cx, cy, 0.1, 10.0)[0]
    rays = full[torch.from_numpy(g["idx"])].contiguous().cuda()
    out = r.render_rays(rays, precision=precision, outputs=("rgb", "depth", "acc", "disp", "z_std", "rgb_coarse", "depth_coarse",
                                                             "acc_coarse", "z_fine", "sample_cond"))
    cliff = np.abs(g["sigma_last_fine"]) < 1e-5
    err = np.abs(out["rgb"].cpu().numpy() - g["rgb_fine"])
    zerr = np.abs(out["z_fine"][:128].cpu().numpy() - g["z_fine_first128"])
    print(f"[{precision} fog] rgb max err", err[~cliff].max(), "depth", np.abs(out["depth"].cpu().numpy() - g["depth_fine"])[~cliff].max(),
          "z_std", np.abs(out["z_std"].cpu().numpy() - g["z_std"]).max(), "z_fine", zerr.max(), "cliff rays", int(cliff.sum()),
          "psnr", psnr(out["rgb"].cpu().numpy(), g["rgb_fine"]))
    assert err[~cliff].max() <= RGB_TOL
    assert np.abs(out["depth"].cpu().numpy() - g["depth_fine"])[~cliff].max() / FAR <= 1e-4
    assert np.abs(out["acc"].cpu().numpy() - g["acc_fine"])[~cliff].max() <= 1e-4
    assert np.abs(out["z_std"].cpu().numpy() - g["z_std"]).max() <= 1e-4
    assert zerr.max() <= 2e-5
    assert np.abs(out["rgb_coarse"].cpu().numpy() - g["rgb_coarse"]).max() <= RGB_TOL
    ratio = out["sample_cond"].cpu().numpy() / g["min_denom"]              # the min over samples may pick a neighbouring bin
    assert np.median(np.abs(ratio - 1)) < 1e-4 and np.abs(ratio - 1).max() < 0.2
    d, dref = out["disp"].cpu().numpy(), g["disp_fine"]
    assert np.array_equal(np.isnan(d)[~cliff], np.isnan(dref)[~cliff])     # acc == 0 -> NaN, as torch.max propagates it
    # disparity = 1/(depth/acc) is a ratio of two sums: compared (relative 1e-3) where acc is not tiny
    ok = ~cliff & ~np.isnan(dref) & (g["acc_fine"] > 1e-2)
    assert (np.abs(d - dref)[ok] / np.abs(dref[ok])).max() <= 1e-3
    assert cliff.sum() <= 4
    r.close()


def test_generic_shape_fp32_against_live_oracle():
    """A shape with no MFMA instantiation (6x64, skip after layer 2, 48+40 samples) through the fp32 kernel,
    checked against the oracle run live on the same rays; the MFMA modes must refuse it loudly."""
    sd_c = nwe_amd.synthetic.thin_fog(nwe_amd.synthetic.make_state_dict(11, 6, 64, skips=(2,)))   # well-conditioned sampling
    sd_f = nwe_amd.synthetic.make_state_dict(12, 6, 64, skips=(2,))
    r = nwe_amd.Renderer(0)
    assert r.set_network(0, sd_c) == (6, 64, 63, 27, 2)
    r.set_network(1, sd_f)
    r.set_sampling(48, 40)
    pose = O.camera_pose((0.3, -0.5, -0.9, 0.0, -90.0, 0.0), (0, 0, 0, 40.0, -10.0, 0.0))
    fx, fy, cx, cy = O.intrinsics(24, 40)
    rays = O.create_rays(pose, 24, 40, fx, fy, cx, cy, 0.1, 10.0)[0]
    ref = O.render_rays(rays, _t(sd_c), _t(sd_f), O.RenderConfig(n_samples=48, n_importance=40))
    out = r.render_rays(rays.cuda(), precision="f32", outputs=("rgb", "depth", "acc", "z_std", "raw_fine", "rgb_coarse"))
    cliff = ref["raw_fine"][:, -1, 3].abs().numpy() < 1e-5
    assert np.abs(out["rgb"].cpu().numpy() - ref["rgb_fine"].numpy())[~cliff].max() <= RGB_TOL
    assert np.abs(out["rgb_coarse"].cpu().numpy() - ref["rgb_coarse"].numpy()).max() <= RGB_TOL
    assert np.abs(out["z_std"].cpu().numpy() - ref["z_std"].numpy()).max() <= 1e-4
    with pytest.raises(NotImplementedError):
        r.render_rays(rays.cuda(), precision="f16x3")
    r.close()


def test_ragged_and_tiny_ray_counts(r_c3):
    """Packets are 128 rays (MFMA) / 16 rays (fp32): counts that are not multiples, a single ray, no rays."""
    fx, fy, cx, cy = O.intrinsics(800, 800)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))
    rays = O.create_rays(pose, 800, 800, fx, fy, cx, cy, 0.1, 10.0)[0][320000:320000 + 300].contiguous().cuda()
    full = r_c3.render_rays(rays, outputs=("rgb", "depth"))
    for n in (1, 31, 33, 129, 299):
        part = r_c3.render_rays(rays[:n].contiguous(), outputs=("rgb", "depth"))
        assert torch.equal(part["rgb"], full["rgb"][:n]) and torch.equal(part["depth"], full["depth"][:n])
    empty = r_c3.render_rays(rays[:0].contiguous(), outputs=("rgb",))
    assert empty["rgb"].shape == (0, 3)


def test_chunking_and_batching_are_result_neutral(r_c3):
    """utils/batch_utils.py:7-25 chunks rays only to bound memory; rays are independent, so any split of the
    frame (row tiles = the multi-GPU shards, or several poses in one launch) must give identical bits."""
    fx, fy, cx, cy = O.intrinsics(48, 64)
    p0 = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, 0.0, 0.0, 0.0))[0].numpy()
    p1 = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -60.0, 0.0, 0.0))[0].numpy()
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth", "acc"))
    whole = r_c3.render(p0, 48, 64, **kw)
    tiles = [r_c3.render(p0, 48, 64, rows=(a, b), **kw) for a, b in ((0, 6), (6, 30), (30, 48))]
    for k in ("rgb", "depth", "acc"):
        assert torch.equal(torch.cat([t[k] for t in tiles]), whole[k])
    both = r_c3.render(np.stack([p0, p1]), 48, 64, **kw)
    other = r_c3.render(p1, 48, 64, **kw)
    assert torch.equal(both["rgb"], torch.cat([whole["rgb"], other["rgb"]]))


def test_c3_full_frame_mfma_against_fp32_kernel():
    """BASELINE config 3 at FULL size (800x800, 64+128, 8x256; 640 000 rays, 1.6e8 MLP evaluations): the MFMA path
    against the on-device fp32 FMA path on every ray -- 150x more rays than the CPU oracle can cover in a test.
    Thin-fog coarse network so that every ray is comparable at full tolerance (see the subset test)."""
    r = nwe_amd.Renderer(0)
    r.set_network(0, nwe_amd.synthetic.thin_fog(_sd(1000, 8, 256)))
    r.set_network(1, _sd(1001, 8, 256))
    r.set_sampling(64, 128)
    fx, fy, cx, cy = O.intrinsics(800, 800)
    pose = O.camera_pose((0.0, -0.5, -0.75 / np.cos(-10 / 180 * np.pi), 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0)
    ref = r.render(pose, 800, 800, precision="f32", outputs=("rgb", "depth", "acc", "raw_fine"), **kw)
    ms32 = r.last_kernel_ms()
    sig_last = ref["raw_fine"][:, -1, 3].abs().cpu().numpy()
    del ref["raw_fine"]
    torch.cuda.empty_cache()
    got = r.render(pose, 800, 800, precision="f16x3", outputs=("rgb", "depth", "acc"), **kw)
    ms = r.last_kernel_ms()
    cliff = sig_last < 1e-5
    err = (got["rgb"] - ref["rgb"]).abs().cpu().numpy()
    print("800x800 mfma vs fp32: rgb max err", err[~cliff].max(), "cliff rays", int(cliff.sum()), "psnr",
          psnr(got["rgb"].cpu().numpy(), ref["rgb"].cpu().numpy()), "kernel ms mfma", ms, "fp32", ms32)
    assert err[~cliff].max() <= RGB_TOL
    assert psnr(got["rgb"].cpu().numpy(), ref["rgb"].cpu().numpy()) > 50
    assert ((got["depth"] - ref["depth"]).abs().cpu().numpy()[~cliff].max()) / FAR <= 1e-4
    assert ((got["acc"] - ref["acc"]).abs().cpu().numpy()[~cliff].max()) <= 1e-4
    assert cliff.sum() <= 64
    assert int(got["flags"].item()) & 0x7 == 0
    fast = r.render(pose, 800, 800, precision="f16x1", outputs=("rgb",), **kw)
    # single-pass fp16 is the fast preview mode (raw sigma error ~1e-3): the last-interval step then flips on rays
    # whose last raw sigma is within a few 1e-3 of zero, so its PSNR is quoted with and without those rays
    wide = sig_last < 5e-3
    p_all = psnr(fast["rgb"].cpu().numpy(), ref["rgb"].cpu().numpy())
    p = psnr(fast["rgb"].cpu().numpy()[~wide], ref["rgb"].cpu().numpy()[~wide])
    print("800x800 single-pass fp16 vs fp32: psnr", p, "(all rays:", p_all, ") rays within 5e-3 of the step:", int(wide.sum()),
          "max err", (fast["rgb"] - ref["rgb"]).abs().cpu().numpy()[~wide].max(), "kernel ms", r.last_kernel_ms())
    assert p > 50 and p_all > 40
    r.close()


def test_c2_coarse_only_400(r_c3):
    """BASELINE config 2 geometry: 400x400, 64 coarse samples, 8x256, no importance pass.  The reference handler
    raises UnboundLocalError with n_importance == 0 (handler.py:263); here the coarse result fills the output slots.
    Checked against the live oracle on a strided subset of the frame, every ray."""
    sd_c = _sd(1000, 8, 256)
    r = nwe_amd.Renderer(0)
    r.set_network(0, sd_c)
    r.set_sampling(64, 0)
    fx, fy, cx, cy = O.intrinsics(400, 400)
    pose = O.camera_pose((0.0, -0.5, -0.75 / np.cos(-10 / 180 * np.pi), 0.0, -90.0, 0.0), (0, 0, 0, 0.0, 0.0, 0.0))
    out = r.render(pose[0].numpy(), 400, 400, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth", "acc", "raw_coarse"))
    assert out["rgb"].shape == (160000, 3)
    idx = torch.arange(0, 160000, 157)
    rays = O.create_rays(pose, 400, 400, fx, fy, cx, cy, 0.1, 10.0)[0][idx].contiguous()
    ref = O.render_rays(rays, _t(sd_c), None, O.RenderConfig(n_samples=64, n_importance=0))
    cliff = ref["raw_coarse"][:, -1, 3].abs().numpy() < 1e-5
    err = np.abs(out["rgb"][idx.cuda()].cpu().numpy() - ref["rgb_coarse"].numpy())
    print("C2 400x400 coarse-only: rgb max err", err[~cliff].max(), "cliff rays", int(cliff.sum()), "kernel ms", r.last_kernel_ms())
    assert err[~cliff].max() <= RGB_TOL
    assert np.abs(out["depth"][idx.cuda()].cpu().numpy() - ref["depth_coarse"].numpy())[~cliff].max() / FAR <= 1e-4
    assert np.abs(out["raw_coarse"][idx.cuda()].cpu().numpy() - ref["raw_coarse"].numpy()).max() < 5e-5
    r.close()


def test_c5_pose_sweep_batch(r_c3):
    """BASELINE config 5 in miniature: a GUI turn-left sweep (30 degree steps, application/app.py:198) rendered as ONE
    batch launch and sharded into row tiles as the multi-GPU path does; tiles and batch must reassemble bit for bit."""
    from nwe_amd.dist import shard_rows
    fx, fy, cx, cy = O.intrinsics(32, 40)
    init = nwe_amd.COORD(x=0.0, y=-0.5, z=-0.76, pitch=-90.0)
    poses = nwe_amd.get_camera_poses_from_list_of_coordinates(init, [nwe_amd.COORD(yaw=-30.0 * k) for k in range(6)]).numpy()
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth", "acc"))
    batch = r_c3.render(poses, 32, 40, **kw)
    rgb = batch["rgb"].reshape(6, 32, 40, 3)
    for k in (0, 3, 5):
        one = r_c3.render(poses[k], 32, 40, **kw)
        assert torch.equal(one["rgb"].reshape(32, 40, 3), rgb[k])
    tiles = [r_c3.render(poses, 32, 40, rows=rr, **kw)["rgb"].reshape(6, rr[1] - rr[0], 40, 3) for rr in shard_rows(32, 3)]
    assert torch.equal(torch.cat(tiles, dim=1), rgb)
    assert (rgb[0] - rgb[3]).abs().max() > 1e-3          # the views differ


def test_workspace_click_render():
    """application/workspace.py:54-68 end to end: floor-plan click -> pose -> uint8 frame."""
    ws = nwe_amd.Workspace("Office Geneve")
    ws.initialize_models(state_dicts=(nwe_amd.synthetic.thin_fog(_sd(1000, 8, 256)), _sd(1001, 8, 256)))
    a = ws.render_image(0.4, 0.6, 0, 0)
    b = ws.render_image(0.4, 0.6, 30, 0)
    assert a.shape == (240, 320, 3) and a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
    assert np.abs(a.astype(int) - b.astype(int)).max() > 0
    init, loc = ws.transform_relative_coordinates(0.4, 0.6, 30, 0)
    assert np.array_equal(ws.handler.render_coordinates(init, loc), b)


def test_to8b_truncates(r_c1):
    x = torch.tensor([-0.5, 0.0, 0.5, 0.999, 1.0, 1.5, 254.9999 / 255.0, 1e-9, 100 / 255.0], device="cuda")
    got = r_c1.to8b(x).cpu().numpy()
    assert np.array_equal(got, O.to8b(x.cpu().numpy()))


def test_handler_drop_in_surface():
    """The reference's three public methods (handler.py:25,88,166) on the 320x240 YAML geometry."""
    h = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "/nonexistent/model.ckpt")
    with pytest.raises(RuntimeError, match="cannot be found"):
        h.initialize_models()
    sd_c = nwe_amd.synthetic.thin_fog(_sd(1000, 8, 256))
    h.initialize_models(state_dicts=(sd_c, _sd(1001, 8, 256)))
    init = nwe_amd.COORD(x=0.0, y=-0.5, z=-0.76, yaw=0.0, pitch=-90.0, roll=0.0)
    img = h.render_coordinates(init, nwe_amd.COORD(yaw=-30.0))
    assert img.dtype == np.uint8 and img.shape == (240, 320, 3) and img.flags["C_CONTIGUOUS"]
    # same pixels through render(): float image, then the reference's to8b (truncation) within +-1
    pose = nwe_amd.get_camera_poses_from_list_of_coordinates(init, [nwe_amd.COORD(yaw=-30.0)])[0].numpy()
    out = h.render(pose)
    assert out["rgb"].shape == (240, 320, 3) and out["depth"].shape == (240, 320)
    assert np.abs(O.to8b(out["rgb"].cpu().numpy()).astype(int) - img.astype(int)).max() == 0
    # against the oracle on a strided subset of this frame
    fx, fy, cx, cy = O.intrinsics(240, 320)
    rays = O.create_rays(torch.from_numpy(pose)[None], 240, 320, fx, fy, cx, cy, 0.1, 10.0)[0]
    idx = torch.arange(0, 240 * 320, 601)
    ref = O.render_rays(rays[idx].contiguous(), _t(sd_c), _t(_sd(1001, 8, 256)), O.RenderConfig())
    cliff = ref["raw_fine"][:, -1, 3].abs().numpy() < 1e-5
    got = out["rgb"].reshape(-1, 3)[idx.cuda()].cpu().numpy()
    assert np.abs(got - ref["rgb_fine"].numpy())[~cliff].max() <= RGB_TOL
    ref8 = O.to8b(ref["rgb_fine"].numpy()).astype(int)
    assert np.abs(img.reshape(-1, 3)[idx.numpy()].astype(int) - ref8)[~cliff].max() <= 1
    d = h._render_rays(rays[idx].contiguous().cuda())
    assert set(d) >= {"rgb_fine", "disp_fine", "acc_fine", "depth_fine", "rgb_coarse", "z_std"}


@pytest.mark.gpu
def test_frame_hand_off_and_preview():
    """render_coordinates writes the truncated uint8 frame (model_utils.py:9) into a caller-owned buffer
    through the pinned staging copy, bit-identical to the fresh-array path; preview=True is the coarse composition
    (handler.py:226-234) and leaves the handler's sampling unchanged."""
    h = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "/nonexistent/model.ckpt")
    sd_c, sd_f = nwe_amd.synthetic.thin_fog(_sd(1000, 8, 256)), _sd(1001, 8, 256)
    h.initialize_models(state_dicts=(sd_c, sd_f))
    init = nwe_amd.COORD(x=0.0, y=-0.5, z=-0.76, yaw=0.0, pitch=-90.0, roll=0.0)
    turn = nwe_amd.COORD(yaw=-60.0)
    fresh = h.render_coordinates(init, turn)
    buf = np.zeros((240, 320, 3), np.uint8)
    ret = h.render_coordinates(init, turn, out=buf)
    assert ret is buf and np.array_equal(buf, fresh)
    again = h.render_coordinates(init, nwe_amd.COORD(yaw=0.0))
    assert not np.array_equal(again, fresh) and np.array_equal(buf, fresh), "a returned frame must not alias the staging buffer"
    with pytest.raises(ValueError):
        h.render_coordinates(init, turn, out=np.zeros((240, 320, 4), np.uint8))
    # preview = coarse pass only: equals rgb_coarse of the full render, and the next full render is unchanged
    prev = h.render_coordinates(init, turn, preview=True)
    pose = nwe_amd.get_camera_poses_from_list_of_coordinates(init, [turn])[0].numpy()
    full = h.render(pose, outputs=("rgb", "rgb_coarse"))
    assert np.array_equal(prev, O.to8b(full["rgb_coarse"].cpu().numpy()))
    assert np.array_equal(h.render_coordinates(init, turn), fresh)


@pytest.mark.gpu
def test_work_decompositions_are_bit_identical():
    """The MFMA kernel has two work decompositions (nwe_mfma_render.h: four ray packets per workgroup, or one packet
    whose samples are dealt to the four waves); the launcher picks by frame size.  Same arithmetic in the same order:
    every output must agree bit for bit, including ragged ray counts and sample counts that are no multiple of four."""
    cases = [(8, 256, 64, 128, 37, 53), (8, 256, 30, 17, 20, 33), (4, 128, 32, 0, 64, 64), (4, 128, 21, 10, 9, 11)]
    names = ("rgb", "depth", "acc", "disp", "z_std", "rgb_coarse", "depth_coarse", "acc_coarse", "raw_coarse", "raw_fine",
             "z_fine", "sample_cond")
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    for D, Wn, ns, ni, H, W in cases:
        r = nwe_amd.Renderer(0)
        r.set_network(0, _sd(1000, D, Wn))
        if ni:
            r.set_network(1, _sd(1001, D, Wn))
        r.set_sampling(ns, ni)
        fx, fy, cx, cy = O.intrinsics(H, W)
        outs = tuple(n for n in names if ni or n in ("rgb", "depth", "acc", "disp", "raw_coarse"))
        res = {}
        for mode in ("0", "1"):
            r.debug_set_decomposition(int(mode))
            for prec in ("f16x3", "f16x1"):
                res[mode, prec] = r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, precision=prec, outputs=outs)
        for prec in ("f16x3", "f16x1"):
            for k in outs:
                a, b = res["0", prec][k], res["1", prec][k]
                assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)), (D, Wn, ns, ni, prec, k)
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_training_mode_forward(golden_dir, precision):
    """SURVEY 8 f4, forward only: stratified jitter (training_handler.py:553-562), sigma noise (model_utils.py:64-71)
    and sample_pdf(det=False) (rays.py:98) on host-drawn random numbers (nwe_set_train_tables), against the oracle's
    training-mode golden (its noise / random-u building blocks are pinned against the reference, the jitter lines are a
    restatement: oracle/make_goldens.py section 9).  Thin-fog coarse net, every ray, both work decompositions."""
    g = np.load(os.path.join(golden_dir, "train_mode.npz"))
    r = nwe_amd.Renderer(0)
    r.set_network(0, nwe_amd.synthetic.thin_fog(_sd(1000, 8, 256)))
    r.set_network(1, _sd(1001, 8, 256))
    r.set_sampling(64, 128)
    fx, fy, cx, cy = O.intrinsics(800, 800)
    full = O.create_rays(torch.from_numpy(g["e2e_pose"])[None], 800, 800, fx, fy, cx, cy, 0.1, 10.0)[0]
    rays = full[torch.from_numpy(g["e2e_idx"])].contiguous().cuda()
    tr = {k: torch.from_numpy(g["e2e_in_" + k]) for k in ("t_rand", "noise_coarse", "noise_fine", "u")}
    outs = ("rgb", "depth", "acc", "z_std", "rgb_coarse", "depth_coarse", "acc_coarse", "z_fine", "sample_cond")
    res = {}
    for mode in (("0", "1") if precision != "f32" else ("0",)):
        r.debug_set_decomposition(int(mode))
        res[mode] = r.render_rays(rays, precision=precision, outputs=outs, train=tr)
    r.debug_set_decomposition(-1)
    out = res["0"]
    if "1" in res:
        for k in outs:
            assert torch.equal(res["0"][k], res["1"][k]), k
    cliff = np.abs(g["e2e_sigma_last_fine"]) < 1e-5
    err = np.abs(out["rgb"].cpu().numpy() - g["e2e_rgb_fine"])
    zerr = np.abs(out["z_fine"][:64].cpu().numpy() - g["e2e_z_fine_first64"])
    print(f"[{precision} train] rgb max err", err[~cliff].max(), "coarse", np.abs(out["rgb_coarse"].cpu().numpy() - g["e2e_rgb_coarse"]).max(),
          "z_fine", zerr.max(), "z_std", np.abs(out["z_std"].cpu().numpy() - g["e2e_z_std"]).max(), "cliff", int(cliff.sum()),
          "min cdf step", float(out["sample_cond"].min()))
    assert np.abs(out["rgb_coarse"].cpu().numpy() - g["e2e_rgb_coarse"]).max() <= RGB_TOL
    assert np.abs(out["depth_coarse"].cpu().numpy() - g["e2e_depth_coarse"]).max() / FAR <= 1e-4
    assert zerr.max() <= 1e-4      # 1e-5 of far; random u and uneven strata are conditioned a little worse than inference (2e-5)
    assert err[~cliff].max() <= RGB_TOL
    assert np.abs(out["depth"].cpu().numpy() - g["e2e_depth_fine"])[~cliff].max() / FAR <= 1e-4
    assert np.abs(out["acc"].cpu().numpy() - g["e2e_acc_fine"])[~cliff].max() <= 1e-4
    assert np.abs(out["z_std"].cpu().numpy() - g["e2e_z_std"]).max() <= 1e-4
    # the tables are one-shot: the next call is plain inference again, and differs
    plain = r.render_rays(rays, precision=precision, outputs=("rgb",))
    assert (plain["rgb"] - out["rgb"]).abs().max().item() > 1e-3
    with pytest.raises(ValueError):
        r.render_rays(rays, precision=precision, train={"t_rand": torch.zeros(3, 64)})
    r.close()


@pytest.mark.gpu
def test_white_background(r_c1):
    """rendering.white_background (model_utils.py:97-98): rgb + (1 - acc), coarse and fine outputs alike."""
    fx, fy, cx, cy = O.intrinsics(16, 16)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "acc", "rgb_coarse", "acc_coarse"))
    plain = r_c1.render(pose, 16, 16, **kw)
    r_c1.set_white_background(True)
    try:
        white = r_c1.render(pose, 16, 16, **kw)
    finally:
        r_c1.set_white_background(False)
    for rgb, acc in (("rgb", "acc"), ("rgb_coarse", "acc_coarse")):
        assert torch.equal(white[acc], plain[acc])
        assert torch.equal(white[rgb], plain[rgb] + (1.0 - plain[acc])[..., None])
    assert torch.equal(r_c1.render(pose, 16, 16, **kw)["rgb"], plain["rgb"])


@pytest.mark.gpu
def test_repeated_renders_are_bit_identical(r_c3):
    """The weight stream is double-buffered through LDS with one barrier per tile and a deliberately relaxed wait in front of
    it (Walker::sync): any race between a late fragment read and the next chunk's DMA would show up as run-to-run
    differences.  Five renders of a frame that fills every CU several times over, both decompositions, every bit equal."""
    fx, fy, cx, cy = O.intrinsics(256, 512)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth", "acc", "rgb_coarse"))
    first = None
    for mode in (0, 1, 2):      # 131072 rays = 4 full rounds of packet workgroups on 256 CUs: plan 2 degenerates to plan 0 here
        r_c3.debug_set_decomposition(mode)
        for _ in range(5 if mode == 0 else 2):
            out = r_c3.render(pose, 256, 512, **kw)
            if first is None:
                first = {k: v.clone() for k, v in out.items()}
            for k in kw["outputs"]:
                assert torch.equal(out[k], first[k]), (mode, k)
    r_c3.debug_set_decomposition(-1)


@pytest.mark.gpu
def test_randomised_sampling_configurations_against_live_oracle():
    """Edge geometry the fixed goldens do not reach: odd and tiny sample counts (Ns=3 is the smallest sample_pdf accepts,
    rays.py:87), the ABI's largest (Ns=128), Ni > Ns, Ni = 1, non-unit ray directions, near/far other than the YAML's, a ragged ray count; MFMA path
    against the oracle run live on the same rays (thin-fog coarse net: well-conditioned sampling, every ray compared)."""
    rng = np.random.default_rng(20240)
    sd_c = nwe_amd.synthetic.thin_fog(_sd(1000, 8, 256))
    sd_f = _sd(1001, 8, 256)
    r = nwe_amd.Renderer(0)
    r.set_network(0, sd_c)
    r.set_network(1, sd_f)
    for ns, ni, near, far, n_rays in [(3, 5, 0.1, 10.0, 70), (5, 1, 0.5, 4.0, 33), (64, 256, 0.1, 10.0, 45), (17, 40, 0.05, 6.0, 129),
                                      (33, 2, 1.0, 2.0, 64), (64, 0, 0.1, 10.0, 50), (4, 0, 0.1, 10.0, 31),
                                      # more than 64 coarse samples: the MFMA kernel's single-packet workgroup (shared cdf buffer)
                                      (128, 128, 0.1, 10.0, 61), (65, 7, 0.2, 5.0, 40), (100, 0, 0.1, 10.0, 33)]:
        r.set_sampling(ns, ni)
        o = rng.uniform(-1.0, 1.0, (n_rays, 3)).astype(np.float32)
        d = (rng.normal(size=(n_rays, 3)) * rng.uniform(0.2, 3.0, (n_rays, 1))).astype(np.float32)   # |d| from 0.2 to ~5
        v = d / np.linalg.norm(d, axis=1, keepdims=True)
        rays = torch.from_numpy(np.concatenate([o, d, np.full((n_rays, 1), near, np.float32), np.full((n_rays, 1), far, np.float32),
                                                v.astype(np.float32)], 1))
        ref = O.render_rays(rays, _t(sd_c), _t(sd_f) if ni else None, O.RenderConfig(n_samples=ns, n_importance=ni))
        for mode in (0, 1):
            r.debug_set_decomposition(mode)
            outs = ("rgb", "depth", "acc") + (("z_fine", "z_std") if ni else ())
            got = r.render_rays(rays.cuda(), precision="f16x3", outputs=outs)
            key = "fine" if ni else "coarse"
            last = ref["raw_" + key][:, -1, 3].abs().numpy()
            ok = last > 1e-5
            err = np.abs(got["rgb"].cpu().numpy() - ref["rgb_" + key].numpy())[ok].max()
            derr = np.abs(got["depth"].cpu().numpy() - ref["depth_" + key].numpy())[ok].max() / far
            assert err <= RGB_TOL and derr <= 1e-4, (ns, ni, mode, err, derr)
            if ni:
                assert np.abs(got["z_fine"].cpu().numpy() - ref["z_fine"].numpy()).max() <= 1e-4 * far, (ns, ni, mode)
                assert np.abs(got["z_std"].cpu().numpy() - ref["z_std"].numpy()).max() <= 1e-4 * far, (ns, ni, mode)
    r.close()


@pytest.mark.gpu
def test_contexts_and_streams_are_independent(r_c1, r_c3):
    """Two contexts with different networks interleaved, and a launch on a non-default torch stream: each result equals
    the one the context produces on its own on the default stream (a context owns its weights, tables and scratch)."""
    fx, fy, cx, cy = O.intrinsics(24, 32)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth"))
    a0 = r_c1.render(pose, 24, 32, **kw)
    b0 = r_c3.render(pose, 24, 32, **kw)
    side = torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(side):
            a = r_c1.render(pose, 24, 32, **kw)
        b = r_c3.render(pose, 24, 32, **kw)
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(a["rgb"], a0["rgb"]) and torch.equal(a["depth"], a0["depth"])
        assert torch.equal(b["rgb"], b0["rgb"]) and torch.equal(b["depth"], b0["depth"])


@pytest.mark.gpu
def test_hybrid_launch_plan(r_c3):
    """A frame with full rounds of 128-ray workgroups plus a ragged rest (300x200 = 60000 rays on 256 CUs: one round of
    32768 rays as packets, 27232 rays sample-split in a second launch): all three plans give the same bits, and the
    launcher's automatic choice is the one its cost model (rounds of workgroups x sample iterations, csrc/nwe_kernel_mfma.hip:
    plan_launch) prescribes - checked as a plan, not as a timing; the times are printed."""
    fx, fy, cx, cy = O.intrinsics(200, 300)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth", "acc", "z_std", "rgb_coarse"))
    res, ms = {}, {}
    for mode in (0, 1, 2, -1):
        r_c3.debug_set_decomposition(mode)
        res[mode] = r_c3.render(pose, 200, 300, **kw)
        torch.cuda.synchronize()
        r_c3.render(pose, 200, 300, **kw)
        ms[mode] = r_c3.last_kernel_ms()
    r_c3.debug_set_decomposition(-1)
    for mode in (1, 2, -1):
        for k in kw["outputs"]:
            assert torch.equal(res[mode][k], res[0][k]), (mode, k)
    print("kernel ms by plan (packets, split, hybrid, auto):", [round(ms[m], 2) for m in (0, 1, 2, -1)])

    def model(n_rays, cus=256, ns=64, ni=128):
        """plan_launch's cost model: rounds of workgroups x sample iterations; two launches for a modelled gain of >= 0.8 %."""
        rounds = lambda rays, per: -(-(-(-rays // per)) // cus)
        its, its_split = ns + ns + ni, 1.06 * ((ns + 3) // 4 + (ns + ni + 3) // 4)
        full = n_rays // 128 // cus * cus * 128
        t_p, t_s = rounds(n_rays, 128) * its, rounds(n_rays, 32) * its_split
        t_h = full // 128 // cus * its + rounds(n_rays - full, 32) * its_split if 0 < full < n_rays else float("inf")
        return 2 if t_h < 0.992 * min(t_p, t_s) else (0 if t_p <= t_s else 1)

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert r_c3.debug_last_plan() == model(200 * 300, cus)
    seen = set()
    for hh, ww in ((64, 64), (240, 320), (100, 800), (203, 131)):   # tiny, the GUI frame, a C4 tile, something ragged
        fx, fy, cx, cy = O.intrinsics(hh, ww)
        r_c3.render(pose, hh, ww, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb",))
        assert r_c3.debug_last_plan() == model(hh * ww, cus), (hh, ww, r_c3.debug_last_plan())
        seen.add(r_c3.debug_last_plan())
    assert cus != 256 or seen == {0, 1, 2}, seen      # on the 256-CU part these sizes exercise all three plans


@pytest.mark.gpu
def test_integration_md_ctypes_stub_runs(r_c3):
    """The ctypes stub printed in INTEGRATION.md section 2 is executed as written (library path substituted, a stand-in
    object with the reference NeRFModel's attribute names) and must reproduce the wrapper's image bit for bit."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    code = re.search(r"```python\nimport ctypes as C.*?```", text, re.S).group(0)[len("```python\n"):-3]
    code = code.replace('C.CDLL("libnwe_hip.so")', f'C.CDLL({nwe_amd._lib.LIB_PATH!r})')

    class FakeModel:                                   # attribute names of nerf/models/nerf_model.py:10-43
        def __init__(self, sd):
            self._sd = {k: torch.from_numpy(v) for k, v in sd.items()}
            self._pts_linears = [None] * 8
            self._W, self._input_ch, self._input_ch_views = 256, 63, 27

        def state_dict(self):
            return self._sd

    ns = {}
    exec(code, ns)
    ns["upload"](0, FakeModel(_sd(1000, 8, 256)))
    ns["upload"](1, FakeModel(_sd(1001, 8, 256)))
    fx, fy, cx, cy = O.intrinsics(16, 24)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    img = ns["render"](pose, 16, 24, fx, fy, cx, cy)
    torch.cuda.synchronize()
    ref = r_c3.render(pose, 16, 24, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb",))["rgb"].reshape(16, 24, 3)
    assert torch.equal(img, ref)
    ns["lib"].nwe_destroy(ns["ctx"])


@pytest.mark.gpu
@pytest.mark.parametrize("D,Wn", [(8, 128), (4, 256), (6, 256), (6, 128)])
def test_further_mfma_shapes(D, Wn):
    """8x128 and 6-deep trunks (skip after layer 4) and 4x256 (no skip layer, as NeRFModel builds it for D <= 5): MFMA instantiations against
    the fp32 kernel and the live oracle on the same rays, both decompositions."""
    sd_c = nwe_amd.synthetic.thin_fog(_sd(1000, D, Wn))
    sd_f = _sd(1001, D, Wn)
    r = nwe_amd.Renderer(0)
    r.set_network(0, sd_c)
    r.set_network(1, sd_f)
    r.set_sampling(64, 128)
    fx, fy, cx, cy = O.intrinsics(20, 24)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))
    rays = O.create_rays(pose, 20, 24, fx, fy, cx, cy, 0.1, 10.0)[0]
    ref = O.render_rays(rays, _t(sd_c), _t(sd_f), O.RenderConfig())
    ok = ref["raw_fine"][:, -1, 3].abs().numpy() > 1e-5
    f32 = r.render_rays(rays.cuda(), precision="f32", outputs=("rgb", "depth"))
    for mode in (0, 1):
        r.debug_set_decomposition(mode)
        got = r.render_rays(rays.cuda(), precision="f16x3", outputs=("rgb", "depth", "raw_coarse"))
        assert np.abs(got["rgb"].cpu().numpy() - ref["rgb_fine"].numpy())[ok].max() <= RGB_TOL
        assert np.abs(got["depth"].cpu().numpy() - ref["depth_fine"].numpy())[ok].max() / FAR <= 1e-4
        assert np.abs(got["raw_coarse"].cpu().numpy() - ref["raw_coarse"].numpy()).max() <= 2e-5
        assert (got["rgb"] - f32["rgb"]).abs().cpu().numpy()[ok].max() <= RGB_TOL
    r.close()


def _rays_from(d, near=0.1, far=10.0):
    """[N,11] rays with origin 0 and the given (unnormalised) directions, the layout of nerf/rays/rays.py:26-30."""
    d = torch.as_tensor(d, dtype=torch.float32)
    n = d.shape[0]
    return torch.cat([torch.zeros(n, 3), d, torch.full((n, 1), near), torch.full((n, 1), far), d / torch.norm(d, dim=-1, keepdim=True)], -1)


@pytest.mark.gpu
@pytest.mark.parametrize("precision,mode", [("f32", -1), ("f16x3", 0), ("f16x3", 1)])
def test_compositing_on_the_reference_edge_vectors(golden_dir, precision, mode):
    """raw2outputs (nerf/models/model_utils.py:49-100) on the device, fed with the reference's own edge vectors through
    nwe_debug_set_raw: sigma <= 0 everywhere (acc = 0, disp = NaN), saturated alpha, sigma_last = +1e-11 / -1e-11 / 1e-9
    (the 1e10 last interval), all-zero sigma; then the same with the sigma noise of the training-mode forward
    (:64-71).  Both kernels, both work decompositions of the MFMA kernel."""
    r = nwe_amd.Renderer(0)
    r.set_network(0, _sd(1000, 4, 128))                      # any network: its outputs are replaced
    r.set_sampling(16, 0)
    r.debug_set_decomposition(mode)
    keys = ("rgb", "disp", "acc", "depth", "weights_coarse", "rgb_coarse")
    g = np.load(os.path.join(golden_dir, "raw2outputs.npz"))
    out = r.render_rays(_rays_from(g["d"]).cuda(), precision=precision, outputs=keys, debug_raw=(torch.from_numpy(g["raw"]), None))
    for k, gk in (("rgb", "rgb"), ("acc", "acc"), ("depth", "depth"), ("weights_coarse", "weights")):
        err = np.abs(out[k].cpu().numpy() - g[gk]).max()
        print(precision, mode, k, err)
        assert err <= 2e-6, (k, err)
    d, dref = out["disp"].cpu().numpy(), g["disp"]
    assert np.array_equal(np.isnan(d), np.isnan(dref)) and np.isnan(dref).sum() >= 2      # sigma <= 0 rows: 1 / max(1e-10, 0/0)
    assert np.allclose(d[~np.isnan(dref)], dref[~np.isnan(dref)], rtol=1e-5)
    assert int(out["flags"].item()) & (1 << 3)                                           # NWE_FLAG_DISP: the reference prints
    # the step at the last interval: sigma_last = 1e-11 -> alpha 0.095..., -1e-11 -> 0, 1e-9 -> 1 - e^-10 (model_utils.py:54)
    w_last = out["weights_coarse"].cpu().numpy()[:, -1]
    assert w_last[4] == 0.0 and w_last[3] > 0.0 and w_last[5] > 0.0                    # sigma_last = -1e-11 / 1e-11 / 1e-9
    t = np.load(os.path.join(golden_dir, "train_mode.npz"))
    out = r.render_rays(_rays_from(t["r2o_d"]).cuda(), precision=precision, outputs=keys, debug_raw=(torch.from_numpy(t["r2o_raw"]), None),
                        train={"noise_coarse": torch.from_numpy(t["r2o_noise"])})
    for k, gk in (("rgb", "r2o_rgb"), ("acc", "r2o_acc"), ("depth", "r2o_depth"), ("weights_coarse", "r2o_weights")):
        assert np.abs(out[k].cpu().numpy() - t[gk]).max() <= 2e-6, k
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision,mode", [("f32", -1), ("f16x3", 0), ("f16x3", 1)])
def test_importance_sampling_on_the_reference_edge_vectors(r_c3, golden_dir, precision, mode):
    """sample_pdf + the sorted merge (nerf/rays/rays.py:74-121, handler.py:243) on the device, fed with the reference's own
    edge vectors through nwe_debug_set_coarse_weights: flat weights, a single spike, ALL-ZERO weights, random, mass at the
    near end, mass in the last bin; u = 1.0 is the last of the 128 arguments of every row.  Then the det=False branch on
    the reference's seeded uniform numbers."""
    g = np.load(os.path.join(golden_dir, "sample_pdf.npz"))
    n = g["weights"].shape[0]
    rays = _rays_from(np.tile(np.array([[0.3, -0.2, 1.0]], np.float32), (n, 1)))
    t = torch.linspace(0., 1., 64)
    z_c = (0.1 * (1. - t) + 10.0 * t).expand(n, 64)
    assert np.array_equal((.5 * (z_c[..., 1:] + z_c[..., :-1])).numpy(), g["bins"])              # the bins the reference was given
    w = torch.zeros(n, 64)
    w[:, 1:-1] = torch.from_numpy(g["weights"])
    w[:, 0], w[:, -1] = 0.25, 0.5                                                               # the end weights are sliced off (handler.py:237)
    r_c3.debug_set_decomposition(mode)
    try:
        out = r_c3.render_rays(rays.cuda(), precision=precision, outputs=("z_fine", "z_std", "sample_cond", "sample_amp", "rgb"),
                               debug_coarse_weights=w)
        want = torch.sort(torch.cat([z_c, torch.from_numpy(g["samples"])], -1), -1).values
        err = (out["z_fine"].cpu() - want).abs().max().item()
        print(precision, mode, "z_fine max err", err)
        assert err <= 1e-6
        assert np.abs(out["z_std"].cpu().numpy() - g["samples"].std(-1)).max() <= 1e-5
        assert torch.isfinite(out["rgb"]).all()
        tm = np.load(os.path.join(golden_dir, "train_mode.npz"))
        w[:, 1:-1] = torch.from_numpy(tm["pdf_weights"])
        out = r_c3.render_rays(rays.cuda(), precision=precision, outputs=("z_fine",), debug_coarse_weights=w,
                               train={"u": torch.from_numpy(tm["pdf_u"])})
        want = torch.sort(torch.cat([z_c, torch.from_numpy(tm["pdf_samples"])], -1), -1).values
        assert (out["z_fine"].cpu() - want).abs().max().item() <= 1e-6
    finally:
        r_c3.debug_set_decomposition(-1)


@pytest.mark.gpu
def test_c4_full_size_row_tiles_equal_the_frame(r_c3):
    """BASELINE config 4 at its stated size on ONE GPU: the 800x800 frame rendered as the 8 row tiles of
    dist.shard_rows(800, 8) - exactly what the 8 ranks render - equals the whole frame bit for bit; each tile's kernel time
    is the per-rank latency of config 4 (80 000 rays = 2.4 rounds of 128-ray workgroups: the launcher renders two rounds as packets
    and the rest sample-split)."""
    from nwe_amd.dist import shard_rows
    fx, fy, cx, cy = O.intrinsics(800, 800)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth", "acc"))
    whole = r_c3.render(pose, 800, 800, **kw)
    t_whole = r_c3.last_kernel_ms()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus != 256 or r_c3.debug_last_plan() == 2   # 5000 workgroups = 19 full rounds as packets + 17 408 rays sample-split (1 % by the model)
    tiles, ms = [], []
    for rr in shard_rows(800, 8):
        tiles.append(r_c3.render(pose, 800, 800, rows=rr, **kw))
        ms.append(r_c3.last_kernel_ms())
        assert r_c3.debug_last_plan() == 2      # 80 000 rays = 2.4 rounds of packets: two full rounds as packets, the rest sample-split
    for k in ("rgb", "depth", "acc"):
        assert torch.equal(torch.cat([t[k] for t in tiles]), whole[k]), k
    # the launches of the last tile, timed apart: two rounds of packets + 14 464 rays sample-split, adding up to the whole
    lp = r_c3.last_launch_parts()
    assert cus != 256 or (len(lp) == 2 and lp[0][1] == 2 * 256 * 128 and lp[0][1] + lp[1][1] == 80000)
    assert all(ms_ > 0 for ms_, _ in lp) and abs(sum(ms_ for ms_, _ in lp) - r_c3.last_kernel_ms()) < 0.05 * r_c3.last_kernel_ms()
    print(f"C4 on one GPU: whole frame {t_whole:.1f} ms; the 8 row tiles {', '.join(f'{m:.1f}' for m in ms)} ms "
          f"(sum {sum(ms):.1f}, slowest {max(ms):.1f} = the frame latency on 8 GPUs before the gather)")
    assert int(whole["flags"].item()) & 0x7 == 0          # rgb, depth, acc finite (disp = 1/(depth/acc) may be NaN where acc = 0, like the reference)
    assert max(ms) < 0.2 * t_whole          # a tile is 1/8 of the rays: not more than 1.6 eighths of the frame's time


@pytest.mark.gpu
def test_c5_full_size_pose_sweep_in_one_launch(r_c3):
    """BASELINE config 5 at its stated size on ONE GPU: 32 poses of the GUI turn-left sweep (11.25 degree steps)
    x 800x800 x (64+128), 8x256, rendered by ONE launch (20.5 M rays, 160 000 workgroups), against per-pose renders."""
    fx, fy, cx, cy = O.intrinsics(800, 800)
    init = nwe_amd.COORD(x=0.0, y=-0.5, z=-0.75 / np.cos(-10.0 / 180.0 * np.pi), pitch=-90.0)
    poses = nwe_amd.get_camera_poses_from_list_of_coordinates(init, [nwe_amd.COORD(yaw=-11.25 * k) for k in range(32)]).numpy()
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth"))
    batch = r_c3.render(poses, 800, 800, **kw)
    ms = r_c3.last_kernel_ms()
    rgb = batch["rgb"].reshape(32, 800 * 800, 3)
    depth = batch["depth"].reshape(32, 800 * 800)
    print(f"C5 on one GPU: 32 frames in one launch {ms:.0f} ms = {32e3 / ms:.2f} frames/s, {32 * 640000 * 192 / (ms * 1e-3):.3e} ray-samples/s")
    for k in (0, 13, 31):
        one = r_c3.render(poses[k], 800, 800, **kw)
        assert torch.equal(one["rgb"], rgb[k]) and torch.equal(one["depth"], depth[k]), k
    assert int(batch["flags"].item()) & 0x7 == 0
    assert (rgb[0] - rgb[16]).abs().max() > 1e-3          # opposite views differ


@pytest.mark.gpu
def test_reference_format_checkpoint_through_the_handler(tmp_path):
    """SURVEY 8(f2) on the device: a checkpoint written the way the reference's training handler writes it
    (nerf_replica_training_handler.py:404-407, keys WITHOUT the leading underscore, handler.py:150-164) is found at
    ckpt_path, loaded by initialize_models() (weights_only=True), and renders the same frame as the same weights passed
    as state dicts."""
    sd_c, sd_f = nwe_amd.synthetic.thin_fog(_sd(21, 8, 256)), _sd(22, 8, 256)
    strip = lambda sd: {k[1:]: torch.from_numpy(v) for k, v in sd.items()}
    path = os.path.join(tmp_path, "model.ckpt")
    torch.save({"global_step": 200000, "network_coarse_state_dict": strip(sd_c), "network_fine_state_dict": strip(sd_f),
                "optimizer_state_dict": {"state": {}, "param_groups": []}}, path)
    h = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", path)
    h.initialize_models()                                                    # no state_dicts=: reads the file
    init = nwe_amd.COORD(x=0.0, y=-0.5, z=-0.76, yaw=0.0, pitch=-90.0, roll=0.0)
    img = h.render_coordinates(init, nwe_amd.COORD(yaw=-30.0))
    h2 = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "unused")
    h2.initialize_models(state_dicts=(sd_c, sd_f))
    assert np.array_equal(img, h2.render_coordinates(init, nwe_amd.COORD(yaw=-30.0)))
    pose = nwe_amd.get_camera_poses_from_list_of_coordinates(init, [nwe_amd.COORD(yaw=-30.0)])[0].numpy()
    assert torch.equal(h.render(pose)["rgb"], h2.render(pose)["rgb"])
    h.initialize_models()                                                    # the GUI calls it on every window open (app.py:116)
    assert np.array_equal(img, h.render_coordinates(init, nwe_amd.COORD(yaw=-30.0)))


@pytest.mark.gpu
def test_one_context_two_streams_back_to_back(r_c3):
    """Launches of ONE context queued on different streams do not share a pose table: two renders with different poses
    issued back to back on two streams give what the same renders give one after the other."""
    fx, fy, cx, cy = O.intrinsics(96, 128)
    p = [O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, a, 0.0, 0.0))[0].numpy() for a in (0.0, -60.0, -120.0)]
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb",))
    want = [r_c3.render(q, 96, 128, **kw)["rgb"].clone() for q in p]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in p]
    got = []
    for _ in range(2):                                   # twice: the second round reuses the slots of the first
        got.clear()
        for q, st in zip(p, streams):
            with torch.cuda.stream(st):
                got.append(r_c3.render(q, 96, 128, **kw)["rgb"])
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_in_process_tiles_through_the_workspace_call():
    """The in-process multi-device path (nwe_render_tiled) behind the reference's synchronous GUI call
    (application/app.py:336 -> Workspace.render_image -> render_coordinates): N contexts in one process, each rendering its
    row tile on its own stream, tiles copied into the frame with hipMemcpyPeerAsync.  On the one-GPU test box the N
    "devices" are the same card ([0, 0, 0] - the same code path as [0, 1, 2]); frames equal the single-context frames bit
    for bit, for ragged tile heights (240 rows over 7 tiles), batches of poses, and through NWE_DEVICES."""
    sds = (nwe_amd.synthetic.thin_fog(_sd(1000, 8, 256)), _sd(1001, 8, 256))
    one = nwe_amd.Workspace("Office Tokyo")
    one.initialize_models(state_dicts=sds)
    want = one.render_image(0.4, 0.6, 30, 0)
    for devices in ([0], [0, 0, 0], [0] * 7):
        ws = nwe_amd.Workspace("Office Tokyo", devices=devices)
        ws.initialize_models(state_dicts=sds)
        got = ws.render_image(0.4, 0.6, 30, 0)
        assert np.array_equal(got, want), devices
        # the frame really went through nwe_render_tiled and EVERY tile rendered (a single-context frame is bit-identical,
        # so equality alone cannot tell; round 2 shipped exactly that silent fallback)
        tr = ws.handler.renderer
        ms = tr.tile_kernel_ms()
        assert tr.last_tiled and len(ms) == len(devices) and all(m > 0 for m in ms), (devices, ms)
        assert tr.peer_access() == [1] * len(devices) and tr.last_warning() == ""
        print("tiles", len(devices), "kernel ms per tile", [round(m, 2) for m in ms])
    # float frames, several poses, depth and acc, non-default size
    init, loc = one.transform_relative_coordinates(0.4, 0.6, 30, 0)
    poses = nwe_amd.get_camera_poses_from_list_of_coordinates(init, [nwe_amd.COORD(yaw=-30.0 * k) for k in range(3)]).numpy()
    a = one.handler.render_batch(poses, 50, 64)
    b = ws.handler.render_batch(poses, 50, 64)
    for k in ("rgb", "depth", "acc"):
        assert torch.equal(a[k], b[k]), k
    assert int(b["flags"].item()) == int(a["flags"].item())
    assert ws.handler.renderer.last_tiled and all(m > 0 for m in ws.handler.renderer.tile_kernel_ms())
    # an explicit full range is the whole frame too; a proper row range takes the single-context path and says so
    c = ws.handler.render_batch(poses, 50, 64, rows=(0, 50))
    assert ws.handler.renderer.last_tiled and torch.equal(c["rgb"], a["rgb"])
    d = ws.handler.render_batch(poses, 50, 64, rows=(10, 20))
    assert not ws.handler.renderer.last_tiled and torch.equal(d["rgb"], a["rgb"][:, 10:20])
    os.environ["NWE_DEVICES"] = "0,0"
    try:
        env = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "unused")          # the reference's two-argument construction
        env.initialize_models(state_dicts=sds)
        assert isinstance(env.renderer, nwe_amd.TiledRenderer) and len(env.renderer.parts) == 2
        assert np.array_equal(env.render_coordinates(init, loc), want)
        assert env.renderer.last_tiled and all(m > 0 for m in env.renderer.tile_kernel_ms())
    finally:
        del os.environ["NWE_DEVICES"]


@pytest.mark.gpu
def test_folded_feature_layer_against_the_unfolded_formulation():
    """The product path multiplies _feature_linear into the view layer at pack time (nerf_model.py:64-70: no activation in
    between; fp64 product on the host).  Against the kernel that evaluates the feature layer as the reference formulates
    it, on the FULL C3 frame (640 000 rays, thin-fog coarse network so that every ray is comparable): raw network outputs
    <= 2e-6, rgb <= 1e-5 on every ray.  The folded stream also evaluates _alpha_linear in fp32 on the vector ALU instead of
    as an MFMA tile, so the two kernels' coarse sigmas differ in the last bits and their importance samples by ~1e-5: the
    fine networks are compared at the SAME depths (the folded run's, fed to both through the debug hook)."""
    sd_c, sd_f = nwe_amd.synthetic.thin_fog(_sd(1000, 8, 256)), _sd(1001, 8, 256)
    fx, fy, cx, cy = O.intrinsics(800, 800)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    res = {}
    for fold in (True, False):
        r = nwe_amd.Renderer(0)
        r.debug_set_fold(fold)
        r.set_network(0, sd_c)
        r.set_network(1, sd_f)
        r.set_sampling(64, 128)
        assert r.packed_stream(0).size == (2080 if fold else 2368) * 1024      # folded: no feature chunks, no alpha tile
        res[fold] = r.render(pose, 800, 800, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth", "acc"))
        ms = r.last_kernel_ms()
        rays = r.create_rays(pose, 800, 800, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, rows=(400, 402))
        if fold:
            z_shared = r.render_rays(rays, outputs=("z_fine",))["z_fine"]
        small = r.render_rays(rays, outputs=("raw_coarse", "raw_fine"), debug_fine_depths=z_shared)
        res[fold].update({k: small[k] for k in ("raw_coarse", "raw_fine")})
        print("folded" if fold else "unfolded", f"{ms:.1f} ms")
        r.close()
    d_rgb = (res[True]["rgb"] - res[False]["rgb"]).abs().max().item()
    d_raw = max((res[True][k] - res[False][k]).abs().max().item() for k in ("raw_coarse", "raw_fine"))
    d_depth = (res[True]["depth"] - res[False]["depth"]).abs().max().item()
    print(f"folded vs unfolded, 640 000 rays: rgb {d_rgb:.2e}, depth {d_depth:.2e}, raw (1600 rays) {d_raw:.2e}")
    assert d_raw <= 2e-6 and d_rgb <= 1e-5 and d_depth / FAR <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_lean_and_full_kernel_instantiations_are_bit_identical(r_c3, mode):
    """A frame that asks for rgb / depth / acc only runs the LEAN instantiation of the MFMA kernel (every other input and
    output compile-time null, no register spills); any further output, a test hook or precomputed rays select the full
    one.  Same arithmetic: identical bits, both work decompositions, both MFMA modes."""
    fx, fy, cx, cy = O.intrinsics(40, 52)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0)
    r_c3.debug_set_decomposition(mode)
    try:
        for precision in ("f16x3", "f16x1"):
            lean = r_c3.render(pose, 40, 52, precision=precision, outputs=("rgb", "depth", "acc"), **kw)
            full = r_c3.render(pose, 40, 52, precision=precision, outputs=("rgb", "depth", "acc", "disp", "z_std", "rgb_coarse", "raw_fine",
                                                                          "weights_coarse", "sample_amp"), **kw)
            rays = r_c3.create_rays(pose, 40, 52, **kw)
            via_rays = r_c3.render_rays(rays, precision=precision, outputs=("rgb", "depth", "acc"))
            for k in ("rgb", "depth", "acc"):
                assert torch.equal(lean[k], full[k]) and torch.equal(lean[k], via_rays[k]), (precision, k)
            assert int(lean["flags"].item()) & 0x7 == int(full["flags"].item()) & 0x7
    finally:
        r_c3.debug_set_decomposition(-1)


@pytest.mark.gpu
def test_handler_renders_any_legal_shape(capsys):
    """The handler's default precision is "auto": the fp32-grade MFMA mode where the shape has an instantiation (8x256 as in
    all four reference YAMLs; also 6-deep, 128-wide ...), else the fp32 vector-ALU HIP kernel with a notice - a legal YAML
    (here net_width 64, net_depth 6) renders instead of raising.  Both against the live oracle."""
    fx, fy, cx, cy = O.intrinsics(12, 16)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))
    rays = O.create_rays(pose, 12, 16, fx, fy, cx, cy, 0.1, 10.0)[0]
    for (D, Wn, skips), want in (((6, 64, (4,)), "f32"), ((6, 256, (4,)), "f16x3"), ((8, 256, (4,)), "f16x3")):
        sd_c = nwe_amd.synthetic.thin_fog(nwe_amd.synthetic.make_state_dict(31, D, Wn, skips=skips))
        sd_f = nwe_amd.synthetic.make_state_dict(32, D, Wn, skips=skips)
        h = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "unused")
        h.initialize_models(state_dicts=(sd_c, sd_f))
        assert h._precision == want
        got = h.render(pose[0].numpy(), 12, 16)["rgb"].reshape(-1, 3).cpu().numpy()
        ref = O.render_rays(rays, _t(sd_c), _t(sd_f), O.RenderConfig())
        ok = ref["raw_fine"][:, -1, 3].abs().numpy() > 1e-5
        assert np.abs(got - ref["rgb_fine"].numpy())[ok].max() <= RGB_TOL, (D, Wn)
        text = capsys.readouterr().out
        assert ("no MFMA instantiation" in text) == (want == "f32")


@pytest.mark.gpu
def test_in_process_tiles_edge_cases():
    """nwe_render_tiled at its edges: more tiles than rows (empty tiles), a context that was never given its networks (the
    call fails on contexts[0] with the tile named, nothing is left writing), and flags from any tile reach the caller."""
    sds = (nwe_amd.synthetic.thin_fog(_sd(1000, 4, 128)), _sd(1001, 4, 128))
    one = nwe_amd.Renderer(0)
    tiled = nwe_amd.TiledRenderer([0] * 5)
    for r in (one, tiled):
        r.set_network(0, sds[0]); r.set_network(1, sds[1]); r.set_sampling(16, 8)
    fx, fy, cx, cy = O.intrinsics(3, 40)
    pose = O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0)
    a, b = one.render(pose, 3, 40, **kw), tiled.render(pose, 3, 40, **kw)          # 3 rows over 5 tiles: two tiles are empty
    for k in ("rgb", "depth", "acc"):
        assert torch.equal(a[k], b[k]), k
    # a NaN network output in the LAST tile's rows only must still set the caller's flag word
    bad = {k: v.copy() for k, v in sds[1].items()}
    bad["_rgb_linear.bias"][:] = np.nan
    for r in (one, tiled):
        r.set_network(1, bad)
    a, b = one.render(pose, 3, 40, **kw), tiled.render(pose, 3, 40, **kw)
    assert int(a["flags"].item()) & 1 and int(b["flags"].item()) == int(a["flags"].item())
    # a context without networks
    broken = nwe_amd.TiledRenderer([0, 0])
    broken.parts[0].set_network(0, sds[0]); broken.parts[0].set_network(1, sds[1])
    for p in broken.parts:
        p.set_sampling(16, 8)
    with pytest.raises(RuntimeError, match="tile 1: .*network not set"):
        broken.render(pose, 3, 40, **kw)
    torch.cuda.synchronize()
    # last_kernel_ms: the last RENDER launch (create_rays does not count) and the calling thread's device is left alone
    ms = one.last_kernel_ms()
    one.create_rays(pose, 3, 40, **kw)
    assert one.last_kernel_ms() == ms and ms > 0
    assert tiled.tile_kernel_ms()[3] < 0 and tiled.tile_kernel_ms()[0] > 0      # tiles 3 and 4 of the 3-row frame never rendered
    assert torch.cuda.current_device() == 0
    for r in (one, tiled, broken):
        r.close()


def _variant_rays(g, use_view_dirs):
    fx, fy, cx, cy = O.intrinsics(800, 800)
    pose = torch.from_numpy(g["novd_pose"])[None]
    return O.create_rays(pose, 800, 800, fx, fy, cx, cy, 0.1, 10.0, use_view_dirs)[0][torch.from_numpy(g["novd_idx"])].contiguous()


def test_networks_without_view_dirs(golden_dir, tmp_path, monkeypatch, capsys):
    """NeRFModel(use_view_dirs=False) (nerf_model.py:41-43,82-83): trunk + _output_linear [5, W], 8-column rays (rays.py:22-30),
    against tests/golden/variants.npz (the reference's own classes): the network alone at the embed.npz points, then 16 + 24
    samples end to end with a thin-fog coarse network (every ray at full tolerance) - through the fp32 HIP kernel and through
    the MFMA kernel's kFormNoViewDirs instantiations (every shape the folded form has; another one asked for explicitly is
    refused, never silently replaced), a 200x200 frame of the MFMA kernel against the fp32 kernel, and the handler with
    rendering.use_view_dirs: False in its YAML."""
    g = np.load(os.path.join(golden_dir, "variants.npz"))
    ge = np.load(os.path.join(golden_dir, "embed.npz"))
    pts = np.concatenate([ge["pts"]] * 2, 0)
    rays_pts = torch.from_numpy(np.concatenate([pts, np.ones_like(pts), np.zeros((pts.shape[0], 2), np.float32)], 1).astype(np.float32)).cuda()
    for tag, D, Wn, seed in (("4x128", 4, 128, 2000), ("8x256", 8, 256, 2001)):
        r = nwe_amd.Renderer(0)
        assert r.set_network(0, nwe_amd.synthetic.make_state_dict(seed, D, Wn, use_view_dirs=False))[3] == 0 and r.ray_columns == 8
        assert r.mfma_supported(0)
        r.set_sampling(2, 0)
        for prec, tol in (("f32", 5e-6), ("f16x3", 5e-6), ("f16x1", 5e-2)):
            for mode in ((-1,) if prec == "f32" else (0, 1)):       # both work decompositions of the MFMA kernel
                r.debug_set_decomposition(mode)
                raw = r.render_rays(rays_pts, precision=prec, outputs=("raw_coarse",))["raw_coarse"].cpu().numpy()
                err = np.abs(raw[:, 0] - g[f"novd_y_{tag}"][:, :4]).max()
                print(f"[no view dirs {tag} {prec} decomposition {mode}] raw vs the reference's NeRFModel: {err:.2e}")
                assert err <= tol
        r.debug_set_decomposition(-1)
        with pytest.raises(ValueError, match="R,8"):
            r.render_rays(torch.zeros(4, 11, device="cuda"), precision="f32")
        r.close()
    sd_c = nwe_amd.synthetic.thin_fog_output(nwe_amd.synthetic.make_state_dict(2001, 8, 256, use_view_dirs=False))
    sd_f = nwe_amd.synthetic.make_state_dict(2002, 8, 256, use_view_dirs=False)
    rays8 = _variant_rays(g, False)
    r = nwe_amd.Renderer(0)
    r.set_network(0, sd_c); r.set_network(1, sd_f); r.set_sampling(16, 24)
    cliff = np.abs(g["novd_sigma_last_fine"]) < 1e-5
    for prec in ("f32", "f16x3"):
        out = r.render_rays(rays8.cuda(), precision=prec, outputs=("rgb", "depth", "acc", "z_std", "rgb_coarse", "depth_coarse", "acc_coarse", "z_fine", "raw_fine"))
        errs = {k: float(np.abs(out[k].cpu().numpy() - g["novd_" + n])[~cliff].max()) for k, n in
                (("rgb", "rgb_fine"), ("depth", "depth_fine"), ("acc", "acc_fine"), ("z_std", "z_std"), ("rgb_coarse", "rgb_coarse"),
                 ("depth_coarse", "depth_coarse"), ("acc_coarse", "acc_coarse"), ("z_fine", "z_fine"))}
        print(f"[no view dirs, end to end, {prec}]", {k: f"{v:.1e}" for k, v in errs.items()})
        assert errs["rgb"] <= RGB_TOL and errs["rgb_coarse"] <= RGB_TOL and errs["depth"] / FAR <= 1e-4 and errs["acc"] <= 1e-4
        assert errs["z_fine"] <= 1e-4 and errs["z_std"] <= 1e-4
        assert np.abs(out["raw_fine"].cpu().numpy()[:32] - g["novd_raw_fine_first32"][..., :4]).max() <= 2e-4   # at slightly moved depths
    # a frame: pinhole rays, the lean instantiation, 64 + 128 samples, the hybrid launch plan - the MFMA kernel against the fp32 kernel
    r.set_sampling(64, 128)
    fx, fy, cx, cy = O.intrinsics(200, 200)
    frame = {prec: r.render(g["novd_pose"], 200, 200, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, precision=prec) for prec in ("f32", "f16x3")}
    plan = r.debug_last_plan()
    d_rgb = (frame["f16x3"]["rgb"] - frame["f32"]["rgb"]).abs().max().item()
    d_depth = (frame["f16x3"]["depth"] - frame["f32"]["depth"]).abs().max().item()
    print(f"[no view dirs, 200x200 frame] MFMA vs fp32 kernel: rgb {d_rgb:.1e}, depth {d_depth:.1e}, launch plan {plan}, "
          f"{r.last_kernel_ms():.2f} ms")
    assert d_rgb <= RGB_TOL and d_depth / FAR <= 1e-4 and frame["f16x3"]["rgb"].std().item() > 0.01
    # repeated, and through the full instantiation (diagnostic outputs requested), and in ONE launch of either decomposition: the same bits
    again = r.render(g["novd_pose"], 200, 200, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, precision="f16x3")
    full = r.render(g["novd_pose"], 200, 200, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, precision="f16x3",
                    outputs=("rgb", "depth", "acc", "z_std", "rgb_coarse"))
    assert all(torch.equal(again[k], frame["f16x3"][k]) and torch.equal(full[k], frame["f16x3"][k]) for k in ("rgb", "depth", "acc"))
    for mode in (0, 1):
        r.debug_set_decomposition(mode)
        one = r.render(g["novd_pose"], 200, 200, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, precision="f16x3")
        assert r.debug_last_plan() == mode and all(torch.equal(one[k], frame["f16x3"][k]) for k in ("rgb", "depth", "acc"))
    r.debug_set_decomposition(-1)
    r.set_sampling(16, 24)
    # create_rays without the view-direction columns: the first eight columns, bit for bit
    fx, fy, cx, cy = O.intrinsics(800, 800)
    mine = r.create_rays(g["novd_pose"], 800, 800, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, rows=(0, 2), use_view_dirs=False)
    assert mine.shape[1] == 8 and torch.equal(mine.cpu(), O.create_rays(torch.from_numpy(g["novd_pose"])[None], 800, 800, fx, fy, cx, cy, 0.1, 10.0, False)[0][:1600])
    # a context must not mix the two kinds of network
    r.set_network(1, nwe_amd.synthetic.make_state_dict(1001, 8, 256))
    with pytest.raises(RuntimeError, match="both have, or both lack"):
        r.render_rays(rays8.cuda(), precision="f32")
    r.close()
    # the other instantiated shapes (no reference vectors for them): the MFMA kernel against the fp32 kernel, which the vectors pin
    for D, Wn, seed in ((6, 256, 2010), (4, 256, 2011), (8, 128, 2012), (6, 128, 2013)):
        r = nwe_amd.Renderer(0)
        r.set_network(0, nwe_amd.synthetic.make_state_dict(seed, D, Wn, use_view_dirs=False)); r.set_sampling(2, 0)
        assert r.mfma_supported(0)
        ref = r.render_rays(rays_pts, precision="f32", outputs=("raw_coarse",))["raw_coarse"]
        for mode in (0, 1):
            r.debug_set_decomposition(mode)
            got = r.render_rays(rays_pts, precision="f16x3", outputs=("raw_coarse",))["raw_coarse"]
            err = (got - ref).abs().max().item()
            print(f"[no view dirs {D}x{Wn} f16x3 decomposition {mode}] raw vs the fp32 kernel: {err:.2e}")
            assert err <= 5e-6
        r.close()
    # a shape without an MFMA instantiation: refused when asked for, the fp32 kernel serves it
    r = nwe_amd.Renderer(0)
    r.set_network(0, nwe_amd.synthetic.make_state_dict(2003, 6, 64, use_view_dirs=False)); r.set_sampling(2, 0)
    assert not r.mfma_supported(0)
    with pytest.raises(NotImplementedError):
        r.render_rays(rays_pts, precision="f16x3", outputs=("raw_coarse",))
    assert torch.isfinite(r.render_rays(rays_pts, precision="f32", outputs=("raw_coarse",))["raw_coarse"]).all()
    r.close()
    # through the handler: a YAML with use_view_dirs: False
    import yaml
    cfg = {k: dict(v) for k, v in nwe_amd.config.INFERENCE_DEFAULTS.items()}
    cfg["rendering"].update(use_view_dirs=False, n_samples=16, n_importance=24)
    cfg["experiment"].update(image_width=24, image_height=16)
    with open(tmp_path / "office_tokyo_config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    monkeypatch.setenv("NWE_CONFIG_DIR", str(tmp_path))
    h = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "synthetic")
    with pytest.raises(RuntimeError, match="view-direction heads"):
        h.initialize_models(state_dicts=(_sd(1000, 8, 256), _sd(1001, 8, 256)))
    h.initialize_models(state_dicts=(sd_c, sd_f))
    said = capsys.readouterr().out
    with capsys.disabled():
        print(said, end="")            # the figures above, visible under -s although this test captures
    assert "no MFMA instantiation" not in said and h._precision == "f16x3"
    res = h._render_rays(rays8.cuda())
    assert np.abs(res["rgb_fine"].cpu().numpy() - g["novd_rgb_fine"])[~cliff].max() <= RGB_TOL
    init, loc = nwe_amd.COORD(x=0.0, y=-0.5, z=-0.76, pitch=-90.0), nwe_amd.COORD(yaw=-30.0)
    img = h.render_coordinates(init, loc)
    pose = nwe_amd.get_camera_poses_from_list_of_coordinates(init, [loc])
    fx, fy, cx, cy = O.intrinsics(16, 24)
    ref = O.render_rays(O.create_rays(pose, 16, 24, fx, fy, cx, cy, 0.1, 10.0, False)[0], _t(sd_c), _t(sd_f), O.RenderConfig(n_samples=16, n_importance=24))
    assert img.shape == (16, 24, 3) and np.abs(img.astype(int) - O.to8b(ref["rgb_fine"].numpy().reshape(16, 24, 3)).astype(int)).max() <= 1


def test_endpoint_feature_map(golden_dir, tmp_path, monkeypatch):
    """experiment.endpoint_feat = True: the fine network is evaluated with show_endpoint (handler.py:248; nerf_model.py:72-81) and
    the view layer's 128 outputs are composited like rgb (model_utils.py:87-89) into feat_map_fine (handler.py:270-271).  The fp32
    HIP kernel against the reference's own result (variants.npz); the MFMA kernel refuses the output; the handler's _render_rays
    carries the key when the YAML says so, and its frames (rgb only) stay on the MFMA kernel."""
    g = np.load(os.path.join(golden_dir, "variants.npz"))
    rays11 = _variant_rays(g, True).cuda()
    sd_c, sd_f = nwe_amd.synthetic.thin_fog(_sd(1000, 8, 256)), _sd(1001, 8, 256)
    r = nwe_amd.Renderer(0)
    r.set_network(0, sd_c); r.set_network(1, sd_f); r.set_sampling(16, 24)
    out = r.render_rays(rays11, precision="f32", outputs=("rgb", "depth", "acc", "feat_map", "z_fine"))
    cliff = np.abs(g["ep_sigma_last_fine"]) < 1e-5
    e_feat = np.abs(out["feat_map"].cpu().numpy() - g["ep_feat_map_fine"])[~cliff]
    print(f"[endpoint_feat] feat_map_fine vs reference: max {e_feat.max():.2e} (|feat| max {np.abs(g['ep_feat_map_fine']).max():.2f}); "
          f"rgb {np.abs(out['rgb'].cpu().numpy() - g['ep_rgb_fine'])[~cliff].max():.2e}, z {np.abs(out['z_fine'].cpu().numpy() - g['ep_z_fine']).max():.1e}")
    assert out["feat_map"].shape == (256, 128)
    assert e_feat.max() <= 1e-4 * max(1.0, float(np.abs(g["ep_feat_map_fine"]).max()))
    assert np.abs(out["rgb"].cpu().numpy() - g["ep_rgb_fine"])[~cliff].max() <= RGB_TOL
    assert np.abs(out["depth"].cpu().numpy() - g["ep_depth_fine"])[~cliff].max() / FAR <= 1e-4
    with pytest.raises(NotImplementedError, match="F32"):
        r.render_rays(rays11, precision="f16x3", outputs=("rgb", "feat_map"))
    r.set_sampling(16, 0)
    with pytest.raises(ValueError, match="n_importance"):
        r.render_rays(rays11, precision="f32", outputs=("rgb", "feat_map"))
    r.close()
    import yaml
    cfg = {k: dict(v) for k, v in nwe_amd.config.INFERENCE_DEFAULTS.items()}
    cfg["rendering"].update(n_samples=16, n_importance=24)
    cfg["experiment"].update(endpoint_feat=True)
    with open(tmp_path / "office_tokyo_config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    monkeypatch.setenv("NWE_CONFIG_DIR", str(tmp_path))
    h = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "synthetic")
    h.initialize_models(state_dicts=(sd_c, sd_f))
    res = h._render_rays(rays11)
    assert np.abs(res["feat_map_fine"].cpu().numpy() - g["ep_feat_map_fine"])[~cliff].max() <= 1e-4 * max(1.0, float(np.abs(g["ep_feat_map_fine"]).max()))
    assert h._precision == "f16x3"                       # frames (rgb only, handler.py:180) keep the MFMA kernel
