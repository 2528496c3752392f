"""The masked reference of the occupancy grid (include/nwe.h: nwe_set_occupancy) and the scenes, grids and networks its tests share.

The rule, in reference terms: run_network's rows of samples whose point lies in a cell marked empty are replaced by zero before
raw2outputs, in the coarse pass (so their weight feeding sample_pdf is 0) and in the fine pass alike.  `masked_render` composes
that from the oracle's own functions in the order of volumetric_rendering; `cell_coords` restates the cell rule in numpy fp32
from the `inv` nwe_get_occupancy reports, so a test computes cells from the very numbers the kernels multiply by.

A sample is DECIDED if, on every axis, its cell coordinate (p - lo) * inv is further than 1e-3 of a cell from an integer: a
kernel whose sample point agrees with the oracle's to ~1e-5 then finds the same cell.  A ray is decided if all its samples
are.  Coarse points are bit-identical to the oracle's (their cells are computed from the fp32 points whatever precision the
reference runs in: the rule is defined on the fp32 point), so only importance samples can be undecided - and each of them is, on
every axis along which the ray sweeps cells, with probability 2e-3 whatever the resolution (the margin is relative to the
cell).  A frame with n_importance samples therefore has about n_importance * 2e-3 * (axes swept) undecided rays: the parity
scenes, which need 95 % decided rays, are the ones with few importance samples (7 + 6) or none (32 + 0); the 64 + 128 and
96 + 32 scenes are held to the identities, which hold on every ray.
"""
import functools

import numpy as np
import torch

import nwe_amd
from oracle import nerf_oracle as O
from tests import early_termination as E

NEAR, FAR = E.NEAR, E.FAR
DECIDED_MARGIN = 1e-3
GROUP = {"packets": (128, 1), "split": (32, 4), "f32": (16, 1)}   # (rays of a group, samples of an iteration): include/nwe.h

# The scene box: every sample of every frame of tests/early_termination.py's cameras (origin (0, -0.77, 0.5), depth 0.1 .. 10)
# lies inside; 2-unit cells.
BOX_LO, BOX_HI, BOX_RES = (-8.0, -2.0, -5.0), (14.0, 16.0, 5.0), (11, 9, 5)
# A box smaller than the scene - it ends at y = 6, which the rays pass at depths of 5 to 18: the samples outside it are
# evaluated whatever its bits say.
SMALL_LO, SMALL_HI, SMALL_RES = (-6.0, -1.0, -4.0), (13.0, 6.0, 4.0), (5, 7, 9)
# The checkerboard's box for the parity scenes WITH importance samples: 1-unit cells around the near part of the rays, which no
# ray's last-but-one coarse sample (depth 8.35 of 7) reaches.  That sample's weight is sample_pdf's last bin, and u = 1 sits on
# the last cdf entry, where one ulp of the cumulative sum decides between `bins[-1]` (cdf[-1] <= 1: denom 0 -> 1, t ~ 0) and
# `bins[-2] + t * width` with t = (1 - cdf[-2]) / (cdf[-1] - cdf[-2]).  With a weight in that bin the two agree to ~1e-6; with the
# bin masked its cdf step is the 1e-5 floor's ~2e-5, and 1e-7 of rounding moves the sample by 1.65 / 2e-5 * 1e-7 ~ 8e-3 units,
# eight times the decided margin.  No other u meets a masked bin but with probability ~2e-5.  So the last bin keeps its weight here,
# as the thin fog keeps `denom < 1e-5` away; tests/test_occupancy_host.py checks it.  Without importance samples (fog32) the checkerboard covers
# the whole scene box.  The quarter-unit offset keeps the cell faces off the planes the cameras' central rays lie in (z = 0.5).
NEAR_LO, NEAR_HI, NEAR_RES = (-5.25, -2.25, -3.25), (3.75, 4.75, 3.75), (9, 7, 7)


def make_grid(bits, lo, hi):
    """A grid as the tests pass it around: bits bool [rx, ry, rz], lo, hi, res and the fp32 inv of nwe_get_occupancy (from a
    host-only context: no device needed)."""
    bits = np.ascontiguousarray(bits, dtype=bool)
    r = nwe_amd.Renderer(host_only=True)
    try:
        r.set_occupancy(bits, lo, hi, bits.shape)
        g = r.occupancy
        assert (r.occupancy_bits() == bits).all()
    finally:
        r.close()
    return {"bits": bits, "lo": np.array(g["lo"], np.float32), "hi": np.array(g["hi"], np.float32), "res": tuple(g["resolution"]),
            "inv": np.asarray(g["inv"], np.float32)}


def cell_centres(lo, hi, res):
    """[rx, ry, rz, 3] float64 centres of the cells (for making grids, not for the rule)."""
    axes = [lo[c] + (np.arange(res[c]) + 0.5) * (hi[c] - lo[c]) / res[c] for c in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1)


def half_space_bits(lo, hi, res, axis=1, above=2.0):
    """Occupied where the cell's centre lies above `above` on `axis`: the near part of every ray is empty."""
    return cell_centres(lo, hi, res)[..., axis] > above


def checkerboard_bits(res, block=2):
    """Blocks of `block` cells, alternately occupied and empty."""
    ix, iy, iz = np.meshgrid(*[np.arange(r) // block for r in res], indexing="ij")
    return (ix + iy + iz) % 2 == 1


def cell_coords(points, grid):
    """points [..., 3] (numpy float32 or float64) -> the cell coordinates (p - lo) * inv in the points' own precision, with the
    fp32 lo and inv: for float32 points this is the kernels' arithmetic, a subtraction and a multiplication rounded to fp32."""
    p = np.asarray(points)
    return (p - grid["lo"].astype(p.dtype)) * grid["inv"].astype(p.dtype)


def classify(points, grid):
    """(empty, decided) per point.  empty: finite, inside the box on every axis, and the cell's bit is 0.  A point that is not
    finite or whose cell index is outside 0 .. r - 1 on any axis is occupied.  decided: see the module docstring (a point that is
    not finite is decided: no rounding brings it back)."""
    c = cell_coords(points, grid)
    with np.errstate(invalid="ignore"):
        f = np.floor(c)
        res = np.array(grid["res"], dtype=c.dtype)
        inside = np.isfinite(c).all(-1) & (f >= 0).all(-1) & (f < res).all(-1)
        idx = np.where(inside[..., None], f, 0).astype(np.int64)
        empty = inside & ~grid["bits"][idx[..., 0], idx[..., 1], idx[..., 2]]
        decided = (~np.isfinite(c) | (np.abs(c - np.round(c)) > DECIDED_MARGIN)).all(-1)
    return empty, decided


def may_be(points, grid):
    """(may be empty, may be occupied) per point: what `classify` says of the point with its cell coordinates moved by up to
    the decided margin on every axis.  A decided point may be only what it is; an undecided one between two cells with the
    same bit likewise."""
    c = cell_coords(points, grid)
    res = np.array(grid["res"], dtype=c.dtype)
    may_empty, may_occupied = np.zeros(c.shape[:-1], bool), np.zeros(c.shape[:-1], bool)
    with np.errstate(invalid="ignore"):
        for dx in (-DECIDED_MARGIN, 0.0, DECIDED_MARGIN):
            for dy in (-DECIDED_MARGIN, 0.0, DECIDED_MARGIN):
                for dz in (-DECIDED_MARGIN, 0.0, DECIDED_MARGIN):
                    f = np.floor(c + np.array([dx, dy, dz], dtype=c.dtype))
                    inside = np.isfinite(c).all(-1) & (f >= 0).all(-1) & (f < res).all(-1)
                    idx = np.where(inside[..., None], f, 0).astype(np.int64)
                    e = inside & ~grid["bits"][idx[..., 0], idx[..., 1], idx[..., 2]]
                    may_empty |= e
                    may_occupied |= ~e
    return may_empty, may_occupied


def masked_render(rays, sd_c, sd_f, cfg, grid, dtype=torch.float32):
    """volumetric_rendering (oracle/nerf_oracle.py) with the raw rows of empty-cell samples replaced by zero in both passes,
    composed from the oracle's functions in its order; grid None = the oracle itself.  Returns rgb / depth / acc of the pass
    that produces the outputs, per pass the samples' empty and decided masks, and per ray `decided`."""
    t = lambda sd: O.cast_state({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, dtype)
    with torch.no_grad():
        rays = rays.to(dtype)
        coarse, fine = t(sd_c), (t(sd_f) if cfg.n_importance > 0 else None)
        rays_o, rays_d = rays[:, 0:3], rays[:, 3:6]
        viewdirs = rays[:, -3:] if rays.shape[-1] > 8 else None
        bounds = rays[..., 6:8].reshape(-1, 1, 2)
        near, far = bounds[..., 0], bounds[..., 1]
        t_vals = torch.linspace(0., 1., steps=cfg.n_samples).to(dtype)
        z_vals = (near * (1. - t_vals) + far * t_vals).expand([rays.shape[0], cfg.n_samples])

        def one_pass(z, state, pts32=None):
            pts = rays_o[..., None, :] + rays_d[..., None, :] * z[..., :, None]
            raw = O.run_network(pts, viewdirs, state, cfg.freqs_xyz, cfg.freqs_dir, cfg.net_chunk)[..., :4]
            if grid is None:
                empty, decided = np.zeros(z.shape, bool), np.ones(z.shape, bool)
                may_empty, may_occupied = empty, ~empty
            elif pts32 is not None:      # the coarse pass: the kernels' own fp32 points, decided by definition
                empty, _ = classify(pts32.numpy(), grid)
                decided, may_empty, may_occupied = np.ones(z.shape, bool), empty, ~empty
            else:
                empty, decided = classify(pts.numpy(), grid)
                may_empty, may_occupied = may_be(pts.numpy(), grid)
            raw = torch.where(torch.from_numpy(empty)[..., None], torch.zeros((), dtype=dtype), raw)
            rgb, _, acc, w, depth = O.raw2outputs(raw, z, rays_d, cfg.white_bkgd)
            return {"rgb": rgb, "acc": acc, "depth": depth, "weights": w, "empty": empty, "decided_samples": decided, "may_empty": may_empty,
                    "may_occupied": may_occupied, "z": z, "raw": raw}

        r32 = rays.to(torch.float32)
        b32 = r32[..., 6:8].reshape(-1, 1, 2)
        t32 = torch.linspace(0., 1., steps=cfg.n_samples)
        z32 = (b32[..., 0] * (1. - t32) + b32[..., 1] * t32).expand([rays.shape[0], cfg.n_samples])
        c = one_pass(z_vals, coarse, r32[:, 0:3][..., None, :] + r32[:, 3:6][..., None, :] * z32[..., :, None])
        out = {"coarse": c}
        last = c
        if cfg.n_importance > 0:
            z_mid = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
            z_samples = O.sample_pdf(z_mid, c["weights"][..., 1:-1], cfg.n_importance)
            z_all, order = torch.sort(torch.cat([z_vals, z_samples], -1), -1)
            last = out["fine"] = one_pass(z_all, fine)
            # the coarse members of the fine depths are the coarse depths, bit for bit: decided like them
            member = (order < cfg.n_samples).numpy()
            last["decided_samples"] = last["decided_samples"] | member
            if grid is not None:
                last["may_empty"] = np.where(member, last["empty"], last["may_empty"])
                last["may_occupied"] = np.where(member, ~last["empty"], last["may_occupied"])
        for k in ("rgb", "depth", "acc"):
            out[k] = last[k]
        out["decided"] = torch.from_numpy(c["decided_samples"].all(-1) & last["decided_samples"].all(-1))
    return out


def executed_interval(ref, kind):
    """[lo, hi] of the ray evaluations a launch of one kind of group may report (nwe_last_ray_evaluations out[0]): per group of
    consecutive rays and per iteration of 1 or 4 samples, in both passes, the group's rays x the iteration's samples unless
    every sample of the iteration is empty.  Undecided samples widen the count to an interval: lo runs an iteration only if a
    sample in it is occupied wherever within the margin its point lies, hi if one may be (may_be)."""
    n_group, per_it = GROUP[kind]
    lo = hi = 0
    for p in ("coarse", "fine"):
        if p not in ref:
            continue
        sure, may = ~ref[p]["may_empty"], ref[p]["may_occupied"]
        n_rays, S = sure.shape
        for g in range(0, n_rays, n_group):
            for s in range(0, S, per_it):
                a, b = sure[g:g + n_group, s:s + per_it], may[g:g + n_group, s:s + per_it]
                lo += a.size if a.any() else 0
                hi += b.size if b.any() else 0
    return lo, hi


def full_evaluations(cfg, n_rays):
    return n_rays * (cfg.n_samples + (cfg.n_samples + cfg.n_importance if cfg.n_importance > 0 else 0))


# ---- the slab network ----------------------------------------------------------------------------------------------------

SLAB_K, SLAB_B = 8.0, -4.8
SLAB_X0 = -10.0 * SLAB_B / SLAB_K        # 6: sigma_raw = relu(k x / 10 + b) is exactly +0 for x <= x0


def slab_state_dict(seed, D, W, use_view_dirs=True):
    """A network whose feature 0 carries t = relu(k x / 10 + b) unchanged through every trunk layer: row 0 of layer 0 is k on
    the identity input x / 10 with bias b, row 0 of every later trunk layer is e_0 (zero on the gamma columns of the skip
    layer) with bias 0, the density head is e_0 with bias 0; every other row is random.  sigma_raw = t, exactly +0 for
    x <= x0 in every precision: zeros split, multiply and accumulate to zero."""
    sd = nwe_amd.synthetic.make_state_dict(seed, D, W, use_view_dirs=use_view_dirs)
    in_xyz = sd["_pts_linears.0.weight"].shape[1]
    sd["_pts_linears.0.weight"][0] = 0.0
    sd["_pts_linears.0.weight"][0, 0] = SLAB_K
    sd["_pts_linears.0.bias"][0] = SLAB_B
    for i in range(1, D):
        w = sd[f"_pts_linears.{i}.weight"]
        w[0] = 0.0
        w[0, in_xyz if w.shape[1] == W + in_xyz else 0] = 1.0
        sd[f"_pts_linears.{i}.bias"][0] = 0.0
    if use_view_dirs:
        sd["_alpha_linear.weight"][:] = 0.0
        sd["_alpha_linear.weight"][0, 0] = 1.0
        sd["_alpha_linear.bias"][:] = 0.0
    else:
        sd["_output_linear.weight"][3] = 0.0
        sd["_output_linear.weight"][3, 0] = 1.0
        sd["_output_linear.bias"][3] = 0.0
    return sd


def slab_grid():
    """The slab's exact grid over the scene box: empty only where the cell lies wholly below x0 - one cell."""
    cell = (BOX_HI[0] - BOX_LO[0]) / BOX_RES[0]
    upper = BOX_LO[0] + (np.arange(BOX_RES[0]) + 1) * cell
    bits = np.broadcast_to((upper > SLAB_X0 - cell)[:, None, None], BOX_RES)
    return make_grid(bits, BOX_LO, BOX_HI)


# ---- scenes --------------------------------------------------------------------------------------------------------------
# name -> (depth, width, n_samples, n_importance, H, W, view dirs, spread).  Fog scenes: a thin-fog coarse network (sigma 0.08,
# acc ~ 0.5) keeps the zero-weight bins the mask creates away from sample_pdf's `denom < 1e-5` switch; the fine network is a
# position-dependent fog (sigma 0.5, spread 3; spread 1, the density head's own gain, where 7 samples are 1.65 units apart: f16x1's
# error in sigma_raw grows with that gain and a weight's with the step.  Measured on an MI355X with NO grid set, f16x1 against the
# f32 kernel: 7 + 6 without view dirs at spread 3 depth 6.2e-3 of its 1e-2, at spread 1 1.2e-3; a 6x128 network without view dirs
# at 32 + 0 and spread 3 rgb 1.25e-3 and acc 1.98e-3, past its 1e-3 before any grid, at spread 1 2.1e-4 and 3.4e-4).
X1_SPREAD = 1.0      # the spread of the scenes that hold f16x1 to its tolerance at coarse steps or over every shape  `fog7`: the split plan's ragged last iteration, one full group and a ragged
# packet; `fog32`: coarse only, 8x256; `fog192`: 64 + 128 on 12 x 64; `fog128`: 96 + 32, more than 64 coarse samples (the
# single-packet workgroup); `novd`: no view directions.
SCENES = {
    "fog7": (4, 128, 7, 6, 7, 19, True, X1_SPREAD),
    "fog32": (8, 256, 32, 0, 7, 19, True, 3.0),
    "fog192": (4, 128, 64, 128, 12, 64, True, 3.0),
    "fog128": (4, 128, 96, 32, 7, 19, True, 3.0),
    "novd": (4, 128, 7, 6, 7, 19, False, X1_SPREAD),
}
PARITY_SCENES = ("fog7", "fog32", "novd")
PARITY_GRIDS = ("half", "checker")


def parity_kind(name, kind):
    """The grid of a parity case: the checkerboard of a scene with importance samples is the one over the near box (NEAR_LO)."""
    return "checker_near" if kind == "checker" and SCENES[name][3] > 0 else kind


@functools.lru_cache(maxsize=None)
def scene(name, n_poses=1):
    """(coarse sd, fine sd, cfg, poses, rays, H, W) of a scene, computed once and shared: leave it unchanged."""
    D, Wd, ns, ni, H, W, vd, spread = SCENES[name]
    S = nwe_amd.synthetic
    if vd:
        sd_c = S.thin_fog(S.make_state_dict(1000, D, Wd))
        sd_f = S.dense_fog(S.make_state_dict(1001, D, Wd), 0.5, spread)
    else:
        sd_c = S.thin_fog_output(S.make_state_dict(1000, D, Wd, use_view_dirs=False))
        sd_f = S.thin_fog_output(S.make_state_dict(1001, D, Wd, use_view_dirs=False), 0.5, spread)
    cfg = O.RenderConfig(n_samples=ns, n_importance=ni)
    poses, rays = E.frame_rays(H, W, n_poses)
    if not vd:
        rays = rays[:, :8].contiguous()
    return sd_c, sd_f, cfg, poses, rays, H, W


@functools.lru_cache(maxsize=None)
def grid(kind):
    if kind == "half":
        return make_grid(half_space_bits(BOX_LO, BOX_HI, BOX_RES), BOX_LO, BOX_HI)
    if kind == "checker":    # 1-unit cells in blocks of two
        res = tuple(2 * r for r in BOX_RES)
        return make_grid(checkerboard_bits(res, 2), BOX_LO, BOX_HI)
    if kind == "checker_near":
        return make_grid(checkerboard_bits(NEAR_RES, 2), NEAR_LO, NEAR_HI)
    if kind == "full":
        return make_grid(np.ones(BOX_RES, bool), BOX_LO, BOX_HI)
    if kind == "none":
        return make_grid(np.zeros(BOX_RES, bool), BOX_LO, BOX_HI)
    if kind == "small_none":
        return make_grid(np.zeros(SMALL_RES, bool), SMALL_LO, SMALL_HI)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def reference(name, kind, fp64=False, n_poses=1):
    """The masked oracle of a scene under a grid (kind None: the plain oracle), shared: leave it unchanged."""
    sd_c, sd_f, cfg, _, rays, _, _ = scene(name, n_poses)
    return masked_render(rays, sd_c, sd_f, cfg, None if kind is None else grid(kind), torch.float64 if fp64 else torch.float32)
