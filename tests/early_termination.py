"""The masked reference of early ray termination (include/nwe.h: nwe_set_early_termination) and the scenes its tests share.

The rule, in reference terms: the outputs of the terminated pass are raw2outputs' with ``weights * (trans >= eps)``, where
``trans`` is the cumprod of nerf/models/model_utils.py:79-80.  `masked_outputs` restates that from the oracle's own ``raw_*`` and
``z_*`` (a NaN ``trans`` is not below eps), and derives what the tests of the skip need: per ray the stop index (the first
sample whose trans is below eps, S if none) and whether the ray is DECIDED - its trans stays further than 1e-3 relative from
eps at every sample, so a kernel whose transmittance agrees with the oracle's to ~1e-5 masks exactly the same samples.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import nwe_amd
from oracle import nerf_oracle as O

NEAR, FAR = 0.1, 10.0
DECIDED_MARGIN = 1e-3


def masked_outputs(raw, z, rays_d, eps, white_bkgd=False):
    """raw [N,S,4], z [N,S], d [N,3] -> dict(rgb, depth, acc, weights, trans, stop, decided); model_utils.py:49-100 with the
    weights of samples whose trans is below eps set to 0.  eps = 0 is raw2outputs."""
    dists = z[..., 1:] - z[..., :-1]
    dists = torch.cat([dists, torch.tensor([1e10], dtype=dists.dtype).expand(dists[..., :1].shape)], -1)
    dists = dists * torch.norm(rays_d[..., None, :], dim=-1)
    rgb = torch.sigmoid(raw[..., :3])
    alpha = 1. - torch.exp(-F.relu(raw[..., 3]) * dists)
    trans = torch.cumprod(torch.cat([torch.ones((alpha.shape[0], 1), dtype=alpha.dtype), 1. - alpha + 1e-10], -1), -1)[:, :-1]
    below = trans < eps                                  # NaN: not below
    zero = torch.zeros((), dtype=alpha.dtype)
    weights = torch.where(below, zero, alpha * trans)
    rgb_map = torch.sum(torch.where(below[..., None], zero, weights[..., None] * rgb), -2)
    depth_map = torch.sum(weights * z, -1)
    acc_map = torch.sum(weights, -1)
    if white_bkgd:
        rgb_map = rgb_map + (1. - acc_map[..., None])
    S = z.shape[-1]
    idx = torch.arange(S).expand(below.shape)
    stop = torch.where(below, idx, torch.full_like(idx, S)).min(-1).values
    decided = ((trans - eps).abs() > DECIDED_MARGIN * eps).all(-1) if eps > 0 else torch.ones(z.shape[0], dtype=torch.bool)
    return {"rgb": rgb_map, "depth": depth_map, "acc": acc_map, "weights": weights, "trans": trans, "stop": stop, "decided": decided}


def frame_rays(H, W, n_poses=1):
    fx, fy, cx, cy = O.intrinsics(H, W)
    poses = torch.cat([O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0.1 * p, 0, 0, -30.0 + 7.0 * p, 0.0, 0.0)) for p in range(n_poses)])
    return poses, O.create_rays(poses, H, W, fx, fy, cx, cy, NEAR, FAR).reshape(-1, 11)


# name -> (depth, width, n_samples, n_importance, sigma, spread, H, W[, coarse sigma, coarse spread]): the scenes of the issue's
# measurements, at frame sizes of a few hundred rays; sigma and spread are the fog (synthetic.dense_fog) of the network of
# the terminated pass, and of the coarse network too unless it has its own.  `mixed`: groups of 128 rays in which some rays stop and some never do, and groups in which all
# stop; `allstop`: every ray stops, 133 rays = one full group of 128 + a ragged packet; `coarse_only`: n_importance == 0;
# `ragged_samples`: sample counts that are no multiple of 4 (the sample-split plan's last iteration), 7 + 6; `thin`: thin_fog, in
# which no transmittance gets anywhere near an eps.
# `mixed` keeps the thin fog in its COARSE network: with the position-dependent density in both networks the importance sampling
# has nearly empty bins and the reference's own fp32 and fp64 results differ by up to 4.4e-4 in rgb on eleven rays (importance
# depths move by 4e-2: DESIGN.md section 6), four times the parity tolerance; with a thin-fog coarse network they agree to
# 5e-7, and the fine network alone decides where rays stop, so the groups are the same.  tests/test_early_termination_host.py
# holds every scene to that: the reference agrees with its own fp64 evaluation to a tenth of the parity tolerance.
SCENES = {
    "mixed": (4, 128, 64, 128, 0.5, 3.0, 12, 64, 0.08, 0.01),
    "allstop": (8, 256, 64, 128, 3.0, 0.01, 7, 19),
    "coarse_only": (8, 256, 32, 0, 0.5, 3.0, 7, 19),
    "ragged_samples": (4, 128, 7, 6, 2.0, 0.01, 7, 19),
    "thin": (4, 128, 64, 128, 0.08, 0.01, 7, 19),
}


@functools.lru_cache(maxsize=None)
def scene(name, H=None, W=None, n_poses=1):
    """(coarse sd, fine sd, cfg, poses, rays, oracle outputs) of a scene, computed once and shared: leave it unchanged."""
    D, Wd, ns, ni, sigma, spread, H0, W0 = SCENES[name][:8]
    c_sigma, c_spread = SCENES[name][8:] or (sigma, spread)
    H, W = H or H0, W or W0
    sd_c = nwe_amd.synthetic.dense_fog(nwe_amd.synthetic.make_state_dict(1000, D, Wd), c_sigma, c_spread)
    sd_f = nwe_amd.synthetic.dense_fog(nwe_amd.synthetic.make_state_dict(1001, D, Wd), sigma, spread)
    cfg = O.RenderConfig(n_samples=ns, n_importance=ni)
    poses, rays = frame_rays(H, W, n_poses)
    t = lambda sd: {k: torch.from_numpy(v) for k, v in sd.items()}
    ref = O.render_rays(rays, t(sd_c), t(sd_f) if ni > 0 else None, cfg)
    return sd_c, sd_f, cfg, poses, rays, ref


def reference_fp64(name):
    """The oracle's fp64 evaluation of a scene (its own error bar: tests/test_early_termination_host.py)."""
    sd_c, sd_f, cfg, _, rays, _ = scene(name)
    t = lambda sd: {k: torch.from_numpy(v) for k, v in sd.items()}
    return O.render_rays(rays, t(sd_c), t(sd_f) if cfg.n_importance > 0 else None, cfg, dtype=torch.float64)


def terminated_pass(ref, cfg):
    """(raw, z) of the pass that produces the outputs: the fine pass, or the only one."""
    return (ref["raw_fine"], ref["z_fine"]) if cfg.n_importance > 0 else (ref["raw_coarse"], ref["z_coarse"])


def masked_reference(name, eps, white_bkgd=False, **kw):
    _, _, cfg, _, rays, ref = scene(name, **kw)
    raw, z = terminated_pass(ref, cfg)
    return masked_outputs(raw, z, rays[:, 3:6], eps, white_bkgd)


def executed_interval(stop, decided, n_rays_group, samples_per_iteration, lag_iterations, S, coarse):
    """[lo, hi] of the ray evaluations a launch may report (nwe_last_ray_evaluations out[0]): per group of `n_rays_group`
    consecutive rays, its rays x (the coarse pass in full + the samples its workgroup walks in the terminated pass).  The
    workgroup needs the largest stop index M of its rays, in whole iterations of `samples_per_iteration`, and may run
    `lag_iterations` more (nwe_mfma_render.h); an undecided ray may stop one sample apart."""
    stop, decided = np.asarray(stop), np.asarray(decided)
    lo = hi = 0
    for g in range(0, len(stop), n_rays_group):
        st, de = stop[g:g + n_rays_group], decided[g:g + n_rays_group]
        n = len(st)
        m_lo = int(np.where(de, st, np.maximum(st - 1, 1)).max())
        m_hi = int(np.where(de, st, np.minimum(st + 1, S)).max())
        its = lambda m, lag: min(S, (-(-m // samples_per_iteration) + lag) * samples_per_iteration)
        lo += n * (coarse + its(m_lo, 0))
        hi += n * (coarse + its(m_hi, lag_iterations))
    return lo, hi
