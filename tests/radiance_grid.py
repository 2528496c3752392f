"""The restated rule of the radiance grid (include/nwe.h: nwe_set_radiance_grid, nwe_render_grid) and the grids its tests share.

`grid_rows` is tests/coarse_grid.py's `grid_sigma` per channel - the coordinate, the inside test, the indices and the fraction are
the coarse grid's - with rows of zeros outside the box: in float32 it gives the bits the kernel interpolates, in float64 the same
function of exact-enough arithmetic.  `grid_render` composes the oracle's own functions in the order of _volumetric_rendering
(handler.py:203-268) with `grid_rows` in run_network's place in BOTH passes:
z_vals -> rows -> raw2outputs -> sample_pdf -> sort -> rows -> raw2outputs.
The scenes, frames and boxes are those of tests/coarse_grid.py.
"""
import functools

import numpy as np
import torch

import nwe_amd
from oracle import nerf_oracle as O
from tests import coarse_grid as B

NEAR, FAR = B.NEAR, B.FAR
BOX_LO, BOX_HI, BOX_RES = B.BOX_LO, B.BOX_HI, B.BOX_RES
SMALL_LO, SMALL_HI, SMALL_RES = B.SMALL_LO, B.SMALL_HI, B.SMALL_RES
H, W, H2, W2 = B.H, B.W, B.H2, B.W2
same_bits = B.same_bits
coarse_points = B.coarse_points


def make_grid(values, lo, hi):
    """A grid as the tests pass it around: values float32 [rx, ry, rz, 4], lo, hi, res and the fp32 inv of nwe_get_radiance_grid
    (from a host-only context: no device needed)."""
    values = np.ascontiguousarray(values, dtype=np.float32)
    r = nwe_amd.Renderer(host_only=True)
    try:
        r.set_radiance_grid(values, lo, hi)
        g = r.radiance_grid
        back = r.radiance_grid_values()
        assert back.shape == values.shape and (back.view(np.uint32) == values.view(np.uint32)).all()
    finally:
        r.close()
    return {"values": values, "lo": np.array(g["lo"], np.float32), "hi": np.array(g["hi"], np.float32), "res": tuple(g["resolution"]),
            "inv": np.asarray(g["inv"], np.float32)}


def channel(grid, c):
    """Channel c of a radiance grid as a coarse grid of tests/coarse_grid.py (3: its sigma channel)."""
    return dict(grid, values=np.ascontiguousarray(grid["values"][..., c]))


def grid_rows(points, grid, dtype=np.float32):
    """points [..., 3] -> rows [..., 4] of the grid there: each channel interpolated on its own, zeros outside the box."""
    return np.stack([B.grid_sigma(points, channel(grid, c), dtype) for c in range(4)], -1)


def grid_render(rays, cfg, grid, dtype=torch.float32):
    """nwe_render_grid in reference terms.  float32: the rows are the fp32 restatement at the kernels' fp32 points; float64: the
    same rule in exact-enough arithmetic, points included.  With n_importance == 0 the only pass is the output."""
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    with torch.no_grad():
        rays = rays.to(dtype)
        rays_o, rays_d = rays[:, 0:3], rays[:, 3:6]
        bounds = rays[..., 6:8].reshape(-1, 1, 2)
        near, far = bounds[..., 0], bounds[..., 1]
        t_vals = torch.linspace(0., 1., steps=cfg.n_samples).to(dtype)
        z_vals = (near * (1. - t_vals) + far * t_vals).expand([rays.shape[0], cfg.n_samples])
        pts = rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]
        raw_c = torch.from_numpy(grid_rows(pts.numpy(), grid, np_dtype))
        rgb, _, acc, w_c, depth = O.raw2outputs(raw_c, z_vals, rays_d, cfg.white_bkgd)
        z_all, raw_f = z_vals, raw_c
        if cfg.n_importance > 0:
            z_mid = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
            z_samples = O.sample_pdf(z_mid, w_c[..., 1:-1], cfg.n_importance)
            z_all, _ = torch.sort(torch.cat([z_vals, z_samples], -1), -1)
            pts_f = rays_o[..., None, :] + rays_d[..., None, :] * z_all[..., :, None]
            raw_f = torch.from_numpy(grid_rows(pts_f.numpy(), grid, np_dtype))
            rgb, _, acc, _, depth = O.raw2outputs(raw_f, z_all, rays_d, cfg.white_bkgd)
    return {"rgb": rgb, "depth": depth, "acc": acc, "weights": w_c, "z_fine": z_all, "raw_fine": raw_f}


# ---- grids ---------------------------------------------------------------------------------------------------------------

def random_rows(res, seed=17, scale=2.0):
    """Random rows of both signs in every channel."""
    rng = np.random.Generator(np.random.Philox(key=[seed, 0]))
    return rng.uniform(-0.5 * scale, scale, size=tuple(res) + (4,)).astype(np.float32)


def smooth_rows(lo, hi, res):
    """The parity scene's rows: tests/coarse_grid.py's thin fog with a soft blob as the density - positive everywhere, so every
    coarse bin carries weight - and a colour that varies smoothly with the position."""
    c = B.G.cell_centres(lo, hi, res)
    colour = np.stack([1.5 * np.sin(0.35 * c[..., 0] + 0.3), 1.2 * np.cos(0.3 * c[..., 1]), 0.8 * np.sin(0.5 * c[..., 2]) - 0.4], -1)
    return np.concatenate([colour, B.smooth_values(lo, hi, res)[..., None]], -1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def grid(kind):
    if kind == "random":             # non-cubic, over the scene box
        return make_grid(random_rows(BOX_RES), BOX_LO, BOX_HI)
    if kind == "small_nonfinite":    # a smaller box that the rays leave, with a NaN, an inf and a -inf in three different channels
        v = random_rows(SMALL_RES, seed=18)
        v[2, 3, 4, 0], v[1, 1, 1, 3], v[3, 5, 7, 2] = np.nan, np.inf, -np.inf
        return make_grid(v, SMALL_LO, SMALL_HI)
    if kind == "smooth":             # the parity scene's: 1-unit cells over the scene box
        res = tuple(2 * r for r in BOX_RES)
        return make_grid(smooth_rows(BOX_LO, BOX_HI, res), BOX_LO, BOX_HI)
    if kind == "one":                # both taps of every axis clamp to the one cell
        return make_grid(random_rows((1, 1, 1), seed=19), SMALL_LO, SMALL_HI)
    if kind == "flat":               # ... of the x axis
        return make_grid(random_rows((1, 7, 2), seed=20), BOX_LO, BOX_HI)
    raise KeyError(kind)


GRIDS = ("random", "small_nonfinite", "smooth", "one", "flat")
PARITY_SCENE, PARITY_GRID = B.PARITY_SCENE, "smooth"


def scene(name, two_poses=False):
    """(cfg, poses, rays, H, W) of a scene of tests/coarse_grid.py: the networks are not needed here."""
    _, _, cfg, poses, rays, h, w = B.scene(name, two_poses)
    return cfg, poses, rays, h, w


@functools.lru_cache(maxsize=None)
def parity_reference(fp64=False):
    """The composed oracle of the parity scene, shared: leave it unchanged."""
    cfg, _, rays, _, _ = scene(PARITY_SCENE)
    return grid_render(rays, cfg, grid(PARITY_GRID), torch.float64 if fp64 else torch.float32)
