"""The restated rule of the baked coarse pass (include/nwe.h: nwe_set_coarse_grid) and the scenes and grids its tests share.

`grid_sigma` restates steps 2 to 4 of the rule in numpy: in float32 - every operation rounded on its own, from the `inv`
nwe_get_coarse_grid reports - it gives the bits the producer kernel gives; in float64 it is the same function of exact
arithmetic, which the host test uses as the error bar of the parity scene.  `coarse_points` restates step 1 (the depths and the
fp32 points the kernels encode).  `baked_render` composes the oracle's own functions in the order of volumetric_rendering:
z_vals -> grid sigma -> raw2outputs -> sample_pdf -> the fine run_network -> raw2outputs.
"""
import functools

import numpy as np
import torch

import nwe_amd
from oracle import nerf_oracle as O
from tests import occupancy as G

NEAR, FAR = G.NEAR, G.FAR
BOX_LO, BOX_HI, BOX_RES = G.BOX_LO, G.BOX_HI, G.BOX_RES          # contains every sample of the shared cameras; (11, 9, 5)
SMALL_LO, SMALL_HI, SMALL_RES = G.SMALL_LO, G.SMALL_HI, G.SMALL_RES   # the rays leave it; (5, 7, 9)


def make_grid(values, lo, hi):
    """A grid as the tests pass it around: values float32 [rx, ry, rz], lo, hi, res and the fp32 inv of nwe_get_coarse_grid
    (from a host-only context: no device needed)."""
    values = np.ascontiguousarray(values, dtype=np.float32)
    r = nwe_amd.Renderer(host_only=True)
    try:
        r.set_coarse_grid(values, lo, hi)
        g = r.coarse_grid
        back = r.coarse_grid_values()
        assert back.shape == values.shape and (back.view(np.uint32) == values.view(np.uint32)).all()
    finally:
        r.close()
    return {"values": values, "lo": np.array(g["lo"], np.float32), "hi": np.array(g["hi"], np.float32), "res": tuple(g["resolution"]),
            "inv": np.asarray(g["inv"], np.float32)}


def grid_sigma(points, grid, dtype=np.float32):
    """points [..., 3] -> sigma_raw [...] of the grid there, in `dtype` arithmetic with the grid's fp32 lo and inv.  float32
    points and dtype: the kernel's bits (numpy rounds every elementwise operation on its own; there is no FMA)."""
    p = np.asarray(points, dtype=dtype)
    lo, inv, v = grid["lo"].astype(dtype), grid["inv"].astype(dtype), grid["values"].astype(dtype)
    res = np.array(grid["res"], dtype=np.int64)
    half = dtype(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        g = (p - lo) * inv - half
        upper = res.astype(dtype) - half
        inside = np.isfinite(p).all(-1) & ~(g < -half).any(-1) & ~(g > upper).any(-1)
        g = np.where(inside[..., None], g, dtype(0))
        fl = np.floor(g)
        f = g - fl
        i0 = np.clip(fl.astype(np.int64), 0, res - 1)
        i1 = np.clip(fl.astype(np.int64) + 1, 0, res - 1)
        lerp = lambda a, b, t: a + (b - a) * t
        x0, y0, z0, x1, y1, z1 = i0[..., 0], i0[..., 1], i0[..., 2], i1[..., 0], i1[..., 1], i1[..., 2]
        fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
        c00, c01 = lerp(v[x0, y0, z0], v[x0, y0, z1], fz), lerp(v[x0, y1, z0], v[x0, y1, z1], fz)
        c10, c11 = lerp(v[x1, y0, z0], v[x1, y0, z1], fz), lerp(v[x1, y1, z0], v[x1, y1, z1], fz)
        out = lerp(lerp(c00, c01, fy), lerp(c10, c11, fy), fx)
    return np.where(inside, out, dtype(0)).astype(dtype)


def coarse_points(rays, n_samples):
    """rays [R, >= 8] float32 (o, d, near, far) -> (z [R, ns], points [R, ns, 3]) in float32, as the kernels form them:
    near * (1 - t) + far * t with torch.linspace's t (handler.py:216-218), then o + d * z, a product and a sum (:223)."""
    rays = np.asarray(rays, dtype=np.float32)
    t = torch.linspace(0., 1., steps=n_samples)
    t, omt = t.numpy(), (1. - t).numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        z = rays[:, 6:7] * omt[None, :] + rays[:, 7:8] * t[None, :]
        pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
    return z.astype(np.float32), pts.astype(np.float32)


def same_bits(a, b):
    """Bit for bit, where a NaN equals a NaN whatever its sign and payload (an x86 inf - inf and the GPU's differ in the sign)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and bool((nan == np.isnan(b)).all()) and bool((a.view(np.uint32)[~nan] == b.view(np.uint32)[~nan]).all())


def baked_render(rays, sd_f, cfg, grid, dtype=torch.float32):
    """The baked call in reference terms, composed from the oracle's functions: rgb / depth / acc of the fine pass, and the
    coarse sigma and weights.  float32: the coarse sigma is the fp32 restatement at the kernels' fp32 points; float64: the same
    rule in exact-enough arithmetic, points included."""
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    with torch.no_grad():
        fine = O.cast_state({k: torch.from_numpy(np.asarray(v)) for k, v in sd_f.items()}, dtype)
        rays = rays.to(dtype)
        rays_o, rays_d = rays[:, 0:3], rays[:, 3:6]
        viewdirs = rays[:, -3:] if rays.shape[-1] > 8 else None
        bounds = rays[..., 6:8].reshape(-1, 1, 2)
        near, far = bounds[..., 0], bounds[..., 1]
        t_vals = torch.linspace(0., 1., steps=cfg.n_samples).to(dtype)
        z_vals = (near * (1. - t_vals) + far * t_vals).expand([rays.shape[0], cfg.n_samples])
        pts = rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]
        sigma = torch.from_numpy(grid_sigma(pts.numpy(), grid, np_dtype))
        raw = torch.cat([torch.zeros(sigma.shape + (3,), dtype=dtype), sigma[..., None]], -1)
        w_c = O.raw2outputs(raw, z_vals, rays_d, cfg.white_bkgd)[3]
        z_mid = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
        z_samples = O.sample_pdf(z_mid, w_c[..., 1:-1], cfg.n_importance)
        z_all, _ = torch.sort(torch.cat([z_vals, z_samples], -1), -1)
        pts_f = rays_o[..., None, :] + rays_d[..., None, :] * z_all[..., :, None]
        raw_f = O.run_network(pts_f, viewdirs, fine, cfg.freqs_xyz, cfg.freqs_dir, cfg.net_chunk)[..., :4]
        rgb, _, acc, _, depth = O.raw2outputs(raw_f, z_all, rays_d, cfg.white_bkgd)
    return {"rgb": rgb, "depth": depth, "acc": acc, "sigma": sigma, "weights": w_c, "z_fine": z_all}


# ---- grids ---------------------------------------------------------------------------------------------------------------

def random_values(res, seed=7, scale=2.0):
    """Random sigma_raw of both signs."""
    rng = np.random.Generator(np.random.Philox(key=[seed, 0]))
    return rng.uniform(-0.5 * scale, scale, size=res).astype(np.float32)


def smooth_values(lo, hi, res):
    """A thin fog with a soft blob in front of the cameras: positive everywhere, so every coarse bin carries weight and
    sample_pdf is well conditioned (nwe_amd.synthetic.thin_fog's argument), and smooth at the cell size."""
    c = G.cell_centres(lo, hi, res)
    d2 = ((c - np.array([2.0, 4.0, 0.5])) ** 2).sum(-1)
    return (0.08 + 0.3 * np.exp(-d2 / (2 * 3.0 ** 2))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def grid(kind):
    if kind == "random":         # non-cubic, over the scene box
        return make_grid(random_values(BOX_RES), BOX_LO, BOX_HI)
    if kind == "small":          # a smaller box that the rays leave
        return make_grid(random_values(SMALL_RES, seed=8), SMALL_LO, SMALL_HI)
    if kind == "small_nonfinite":   # ... with a NaN and an inf among its values
        v = random_values(SMALL_RES, seed=8)
        v[2, 3, 4], v[1, 1, 1], v[3, 5, 7] = np.nan, np.inf, -np.inf
        return make_grid(v, SMALL_LO, SMALL_HI)
    if kind == "smooth":         # the parity scene's: 1-unit cells over the scene box
        res = tuple(2 * r for r in BOX_RES)
        return make_grid(smooth_values(BOX_LO, BOX_HI, res), BOX_LO, BOX_HI)
    raise KeyError(kind)


# ---- scenes --------------------------------------------------------------------------------------------------------------
# name -> (depth, width, n_samples, n_importance, view dirs, fine fog's spread).  Frames are 13 x 37 (481 rays: ragged for
# 128-ray and for 32-ray work items) or 2 poses of 9 x 16.  The fine network is synthetic.dense_fog(0.5, spread); the spread of
# the parity scene is the one at which f16x1 meets its tolerance at 7 coarse samples (tests/occupancy.py: X1_SPREAD).
SCENES = {
    "s7": (4, 128, 7, 6, True, G.X1_SPREAD),
    "s192": (4, 128, 64, 128, True, 3.0),
    "s128": (4, 128, 96, 32, True, 3.0),
    "big7": (8, 256, 7, 6, True, G.X1_SPREAD),
    "novd": (4, 128, 7, 6, False, G.X1_SPREAD),
}
H, W = 13, 37
H2, W2 = 9, 16
PARITY_SCENE, PARITY_GRID = "s7", "smooth"


@functools.lru_cache(maxsize=None)
def scene(name, two_poses=False):
    """(coarse sd, fine sd, cfg, poses, rays, H, W) of a scene, computed once and shared: leave it unchanged."""
    D, Wd, ns, ni, vd, spread = SCENES[name]
    S = nwe_amd.synthetic
    if vd:
        sd_c = S.thin_fog(S.make_state_dict(1000, D, Wd))
        sd_f = S.dense_fog(S.make_state_dict(1001, D, Wd), 0.5, spread)
    else:
        sd_c = S.thin_fog_output(S.make_state_dict(1000, D, Wd, use_view_dirs=False))
        sd_f = S.thin_fog_output(S.make_state_dict(1001, D, Wd, use_view_dirs=False), 0.5, spread)
    cfg = O.RenderConfig(n_samples=ns, n_importance=ni)
    h, w = (H2, W2) if two_poses else (H, W)
    poses, rays = G.E.frame_rays(h, w, 2 if two_poses else 1)
    if not vd:
        rays = rays[:, :8].contiguous()
    return sd_c, sd_f, cfg, poses, rays, h, w


@functools.lru_cache(maxsize=None)
def parity_reference(fp64=False):
    """The composed oracle of the parity scene, shared: leave it unchanged."""
    _, sd_f, cfg, _, rays, _, _ = scene(PARITY_SCENE)
    return baked_render(rays, sd_f, cfg, grid(PARITY_GRID), torch.float64 if fp64 else torch.float32)
