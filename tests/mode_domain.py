"""The three opt-in render modes - early ray termination, the shared coarse pass, separate passes (include/nwe.h) - over every
network shape their kernels are built for and over the degenerate inputs of tests/input_domain.py: the shape list, the
scenes, the CPU references and the expectations shared by tests/test_mode_domain_host.py (CPU) and
tests/test_gpu_mode_domain.py (GPU).  Nothing here needs a GPU.

Part A: the 12 shapes (six folded, six without view directions) on a 7 x 19 frame of two poses - 266 rays: two full groups of
128 rays and a ragged packet - in three fog scenes.  Part B: the 16 pinhole cases of tests/input_domain.py on three shapes.
"""
import functools

import numpy as np
import torch

from nwe_amd import synthetic
from oracle import nerf_oracle as O
from tests import early_termination as E
from tests import input_domain as I
from tests import shared_coarse as SC

# ---- shapes ---------------------------------------------------------------------------------------------------------------------
# every (D, W) the terminating and the sharing kernels are built for (nwe_mfma_shapes.h: every shape but the reference
# formulation), listed as tests/test_gpu_accuracy.py lists INSTANTIATIONS; tests/test_mode_domain_host.py holds the list to that
# one and to what the packer accepts
FOLDED = [(8, 256), (4, 128), (8, 128), (4, 256), (6, 256), (6, 128)]
NO_VIEW_DIRS = [(8, 256), (4, 128), (6, 256), (4, 256), (8, 128), (6, 128)]
SHAPES = [(D, W, "folded") for D, W in FOLDED] + [(D, W, "no_view_dirs") for D, W in NO_VIEW_DIRS]


def kind(D, W, form):
    """The name the mode tests give a shape: '6x128', '6x128-noview'."""
    return f"{D}x{W}" + ("-noview" if form == "no_view_dirs" else "")


IDS = [kind(*s) for s in SHAPES]
NETS = {kind(D, W, form): (D, W, form != "no_view_dirs") for D, W, form in SHAPES}       # name -> (depth, width, view directions)
# separate passes, two shapes: every ordered pair of neighbours on a ring through all six, per formulation
RING = [(8, 256), (6, 128), (4, 256), (8, 128), (6, 256), (4, 128)]
PAIRS = []
for _form in ("folded", "no_view_dirs"):
    for _i in range(6):
        _a, _b = kind(*RING[_i], _form), kind(*RING[(_i + 1) % 6], _form)
        PAIRS += [(_a, _b), (_b, _a)]
# the shapes of the large sample counts and of part B
COUNT_SHAPES = [(8, 256, "folded"), (6, 128, "folded"), (4, 128, "no_view_dirs")]
BIG_COUNTS = [(96, 32), (65, 7), (128, 256)]         # more than 64 coarse samples: sample split only; the last is the ABI maximum
DOMAIN_SHAPES = [(8, 256, "folded"), (6, 256, "folded"), (4, 128, "no_view_dirs")]

H, W, N_POSES = 7, 19, 2
N_RAYS = H * W * N_POSES
LEAN = ("rgb", "depth", "acc")


def density_only(D, Wd, form):
    """Whether the coarse pass of a lean frame evaluates the density alone (nwe_mfma_eval.h: density_only_built): folded
    networks but the 6-deep ones, whose gamma(x) skip input enters the last trunk layer - those keep the coarse colour and
    report NWE_FLAG_RGB_COARSE, like the networks without view directions (one head for colour and density)."""
    return form == "folded" and D != 6


# ---- part A: scenes -------------------------------------------------------------------------------------------------------------
# name -> ((coarse sigma, spread), (fine sigma, spread), eps).  `thin`: no transmittance gets near 1e-4, the terminating
# kernel masks nothing; `halfstop`: a nearly uniform fine fog in which |d| of the pixel decides whether a ray stops - the image
# edges stop, the centre does not, in every 128-ray group; `allstop`: every ray stops (at 7 + 6 the sample-split plan's last
# iteration is ragged).  The coarse network stays thin in all three so that the importance sampling is well conditioned
# (tests/early_termination.py on its scene `mixed`); with the dense fog in both networks up to 6 % of the rays of `allstop` are
# undecided at 7 + 6, with the thin coarse fog none is.
SCENES = {"thin": ((0.08, 0.01), (0.08, 0.01), 1e-4),
          "halfstop": ((0.08, 0.01), (0.4, 0.01), 1e-2),
          "allstop": ((0.08, 0.01), (3.0, 0.01), 1e-2)}


def tensors(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def fog_nets(D, Wd, form, name):
    """Networks 1000 / 1001 of the shape (the seeds of every mode test) with the density heads of scene `name`."""
    view = form != "no_view_dirs"
    fog = synthetic.thin_fog if view else synthetic.thin_fog_output
    c, f, _ = SCENES[name]
    return (fog(synthetic.make_state_dict(1000, D, Wd, use_view_dirs=view), *c),
            fog(synthetic.make_state_dict(1001, D, Wd, use_view_dirs=view), *f))


@functools.lru_cache(maxsize=None)
def frame(view=True):
    """(poses, rays) of the 7 x 19 frame of two poses; 8 columns without view directions (nerf/rays/rays.py:22-30)."""
    poses, rays = E.frame_rays(H, W, N_POSES)
    return poses, (rays if view else rays[:, :8].contiguous())


@functools.lru_cache(maxsize=None)
def scene(D, Wd, form, name, ns=64, ni=128, dtype=torch.float32):
    """(coarse sd, fine sd, cfg, poses, rays, oracle outputs) - computed once and shared: leave it unchanged."""
    sd_c, sd_f = fog_nets(D, Wd, form, name)
    cfg = O.RenderConfig(n_samples=ns, n_importance=ni)
    poses, rays = frame(form != "no_view_dirs")
    ref = O.render_rays(rays, tensors(sd_c), tensors(sd_f), cfg, dtype=dtype,
                        keep=("raw_fine", "z_fine", "rgb_fine", "depth_fine", "acc_fine"))
    return sd_c, sd_f, cfg, poses, rays, ref


def masked_reference(D, Wd, form, name, ns=64, ni=128, eps=None, dtype=torch.float32):
    """E.masked_outputs on the fine pass of the scene; eps defaults to the scene's."""
    _, _, _, _, rays, ref = scene(D, Wd, form, name, ns, ni, dtype)
    return E.masked_outputs(ref["raw_fine"][..., :4], ref["z_fine"], rays[:, 3:6].to(dtype), SCENES[name][2] if eps is None else eps)


TOL = {"rgb": 1e-4, "depth": 1e-4 * E.FAR, "acc": 1e-4}        # the parity tolerances of tests/test_gpu_early_termination.py


def per_ray(err):
    return err.max(-1).values if err.dim() == 2 else err


def scene_figures(D, Wd, form, name, ns=64, ni=128):
    """What the conditions of the host test are made of, from the CPU oracle alone: the share of rays that stop and of
    undecided rays, the largest |masked - plain| per output, and the largest |fp32 - fp64| of the masked reference on the rays
    decided in both."""
    eps = SCENES[name][2]
    m = masked_reference(D, Wd, form, name, ns, ni)
    plain = masked_reference(D, Wd, form, name, ns, ni, eps=0.0)
    m64 = masked_reference(D, Wd, form, name, ns, ni, dtype=torch.float64)
    S = ns + ni
    both = m["decided"] & m64["decided"]
    fig = {"stop": float((m["stop"] < S).float().mean()), "undecided": float((~m["decided"]).float().mean()),
           "decided_both": float(both.float().mean()), "eps": eps}
    for k in LEAN:
        fig["bite_" + k] = float(per_ray((m[k] - plain[k]).abs()).max())
        fig["bite_min_" + k] = float(per_ray((m[k] - plain[k]).abs())[m["stop"] < S].min()) if fig["stop"] > 0 else 0.0
        fig["fp64_" + k] = float(per_ray((m[k].double() - m64[k]).abs())[both].max()) if both.any() else 0.0
    return fig


def intervals(stop, decided, ns, S, lag):
    """plan -> (lo, hi) of nwe_last_ray_evaluations out[0]: packets (groups of 128 rays, a sample per iteration), sample split
    (groups of 32, four samples; the hybrid plan of a frame below one full round of packet workgroups is all sample split) and
    the fp32 kernel (groups of 16, no lag).  `lag`: tests/test_gpu_early_termination.LAG."""
    return {"packets": E.executed_interval(stop, decided, 128, 1, lag["packets"], S, ns),
            "split": E.executed_interval(stop, decided, 32, 4, lag["split"], S, ns),
            "f32": E.executed_interval(stop, decided, 16, 1, lag["f32"], S, ns)}


# ---- the GPU-side expectations of the rules, from calls that exist without the modes -------------------------------------------

def camera(h=H, w=W):
    fx, fy, cx, cy = O.intrinsics(h, w)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=E.NEAR, far=E.FAR)


def expected_shared(r, poses, h, w, k, precision, view=True, cam=None):
    """The shared coarse pass, from entry points that exist without it: (a) the ordinary render's fine depths Z of the frame's
    rays, (b) every ray's fine pass on Z[rep].  The context `r` (a Renderer on a GPU) must have k = 1 while this runs."""
    cam = camera(h, w) if cam is None else cam
    n_poses = np.asarray(poses).reshape(-1, 4, 4).shape[0]
    rays = r.create_rays(poses, h, w, use_view_dirs=view, **cam)
    Z = r.render_rays(rays, precision=precision, outputs=LEAN + ("z_fine",))["z_fine"]
    rep = torch.from_numpy(SC.rep_index(h, w, k, 0, h, n_poses)).to(Z.device)
    return r.render_rays(rays, precision=precision, outputs=LEAN, debug_fine_depths=Z[rep].contiguous())


def expected_mixed(make, coarse, fine, precision, rays, coarse_outputs, rest_outputs):
    """Separate passes on two shapes: context A = make(coarse, coarse) gives the coarse outputs and weights; context
    B = make(fine, fine) everything else, on A's weights through the coarse-weights hook.  Both render with the fused kernels.
    `make(c, f)`: a renderer with network c (seed 1000) in slot 0 and f (seed 1001) in slot 1, a (name, seed) pair to put the
    other seed's network there."""
    A, B = make(coarse, (coarse, 1000)), make((fine, 1001), fine)
    try:
        a = A.render_rays(rays, precision=precision, outputs=coarse_outputs)
        b = B.render_rays(rays, precision=precision, outputs=rest_outputs, debug_coarse_weights=a["weights_coarse"])
        return a, b
    finally:
        A.close(); B.close()


# ---- part B: the input-domain table ---------------------------------------------------------------------------------------------
DOMAIN_CASES = [c.name for c in I.CASES if c.pose is not None]          # the 16 pinhole cases
FINITE_DEPTHS = [n for n in DOMAIN_CASES if n not in ("far_inf", "nan_c2w")]
FINE_FOG = (0.4, 0.01)                                                 # B3: rays stop at eps = 1e-2
DOMAIN_EPS = 1e-2


@functools.lru_cache(maxsize=None)
def domain_oracle(name, D, Wd, form, fine_fog=None):
    """(rays, coarse sd, fine sd, oracle outputs) of a case of tests/input_domain.py; leave it unchanged."""
    with np.errstate(all="ignore"):
        return I.run_oracle(I.BY_NAME[name], D, Wd, form, fine_fog=fine_fog)


def fine_pass(rays, z_all, sd_f, cfg=None):
    """O.fine_pass_given_depths for rays with or without view directions."""
    cfg = cfg or O.RenderConfig(n_samples=I.NS, n_importance=I.NI)
    viewdirs = rays[:, -3:] if rays.shape[-1] > 8 else None
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z_all[..., :, None]
    with torch.no_grad():
        raw = O.run_network(pts, viewdirs, tensors(sd_f), cfg.freqs_xyz, cfg.freqs_dir, cfg.net_chunk)
        rgb, disp, acc, w, depth = O.raw2outputs(raw, z_all, rays[:, 3:6], cfg.white_bkgd)
    return {"rgb": rgb, "depth": depth, "acc": acc, "disp": disp}


def domain_shared_reference(name, D, Wd, form, k):
    """The oracle-side shared reference of a case: sample_pdf on weights[rep] is z_fine[rep] (the coarse depths are the
    frame's), then every ray's own fine pass on those depths - as SC.shared_reference does for its scenes."""
    rays, _, sd_f, res = domain_oracle(name, D, Wd, form)
    rep = torch.from_numpy(SC.rep_index(I.H, I.W, k, 0, I.H, 1))
    return fine_pass(rays, res["z_fine"][rep], sd_f)


def domain_masked_reference(name, D, Wd, form, eps=DOMAIN_EPS):
    """B3: E.masked_outputs on the oracle's raw_fine / z_fine of the case with the fine fog."""
    rays, _, _, res = domain_oracle(name, D, Wd, form, FINE_FOG)
    return E.masked_outputs(res["raw_fine"][..., :4], res["z_fine"], rays[:, 3:6], eps)
