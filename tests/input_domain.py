"""Degenerate and non-finite inputs: one table of named cases shared by tests/test_input_domain_oracle.py (CPU) and
tests/test_gpu_input_domain.py (GPU), like tests/accuracy.py is shared by the accuracy tests.

A case gives rays (a pinhole pose + frame, so that nwe_render / nwe_render_tiled and their lean frames can run it too, or an
explicit ray table), a way to spoil the two networks, the sampling, and a HAND-WRITTEN expectation: for every output of
OUTPUTS, which rays hold a non-finite element.  The expectation is what the reference does on such input (it prints
"[Numerical Error] <key> contains NaN or inf.", handler.py:273-275); the CPU test checks it against the fp32 oracle, the GPU
test checks the kernels against the oracle per element.

`expected_flags` turns oracle outputs into the NWE_FLAG_* word include/nwe.h promises for a set of requested outputs.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from nwe_amd import synthetic
from oracle import nerf_oracle as O

# include/nwe.h
FLAG_RGB, FLAG_DEPTH, FLAG_ACC, FLAG_DISP = 1, 2, 4, 8
FLAG_RGB_COARSE, FLAG_DEPTH_COARSE, FLAG_ACC_COARSE, FLAG_DISP_COARSE = 16, 32, 64, 128
FLAG_RAW, FLAG_ZSTD = 256, 512

# kernel output name -> oracle key (fine pass); without importance samples the "fine" slots hold the coarse results
PER_RAY_FINE = {"rgb": "rgb_fine", "depth": "depth_fine", "acc": "acc_fine", "disp": "disp_fine"}
PER_RAY_COARSE = {"rgb_coarse": "rgb_coarse", "depth_coarse": "depth_coarse", "acc_coarse": "acc_coarse", "disp_coarse": "disp_coarse"}
PER_SAMPLE = {"raw_coarse": "raw_coarse", "raw_fine": "raw_fine", "z_fine": "z_fine"}
OUTPUTS = tuple(PER_RAY_FINE) + ("z_std",) + tuple(PER_RAY_COARSE) + tuple(PER_SAMPLE)
FINE_SIDE = tuple(PER_RAY_FINE) + ("z_std", "raw_fine", "z_fine")
COARSE_SIDE = tuple(PER_RAY_COARSE) + ("raw_coarse",)
FULL = OUTPUTS                                   # what a full frame requests
LEAN = ("rgb", "depth", "acc")                   # what a lean frame requests (nwe_render only: precomputed rays are never lean)

ALL = "all"
ACC0 = "acc0"                                    # the rays whose acc of that pass is exactly 0: disp = 1 / max(1e-10, 0 / 0) = NaN
Rays = Union[str, Sequence[int]]                 # ALL, ACC0 or a list of ray indices


def _pose(yaw_deg: float = -30.0) -> np.ndarray:
    return O.camera_pose((0.0, -0.5, -0.76, 0.0, -90.0, 0.0), (0, 0, 0, yaw_deg, 0.0, 0.0))[0].numpy().astype(np.float32)


H, W = 6, 8                                      # pinhole cases: 48 rays, two tiles of three rows in nwe_render_tiled
# Value comparisons take max / p99 / median over the rays: over 48 rays those are single rays (measured there: f16x3 up to 2.2 x
# the yardstick on max with the median at 1.0), so they run on 1536 rays, as the end-to-end tests of test_gpu_accuracy.py run
# on 2048 or more.
BIG_H, BIG_W = 32, 48
BIG_RAYS = BIG_H * BIG_W + 6                     # ray tables: three packets more than full rounds, the last one ragged
NEAR, FAR = 0.1, 10.0
# nwe_selftest report[7] (1e-9 units): the reference's own sinf / cosf error over the positional encoding's documented range plus
# one fp32 ulp; tests/test_input_domain_oracle.py derives it, tests/test_gpu_parity.py asserts it
SINCOS_WIDE_BOUND = 100


@dataclass
class Case:
    name: str
    expect: Dict[str, Rays]                      # output -> rays with a non-finite element; outputs not named: none, but
                                                 # disp / disp_coarse: ACC0 (model_utils.py:94 on a ray that met no density)
    pose: Optional[np.ndarray] = None            # pinhole case: c2w [4,4] of an H x W frame
    near: float = NEAR
    far: float = FAR
    rays: Optional[Callable[[bool], torch.Tensor]] = None    # explicit rays: use_view_dirs -> [R, 11 | 8]
    spoil: Optional[Tuple[str, str, Tuple[int, ...], float]] = None   # (network "coarse" | "fine", key, index, value)
    spoil_novd: Optional[Tuple[str, str, Tuple[int, ...], float]] = None   # the same for networks without view directions
    expect_novd: Optional[Dict[str, Rays]] = None            # expectation without view directions, where it differs
    values: bool = False                         # all-finite case whose values are held to the criterion of tests/accuracy.py
    f32_overflow: bool = False                   # the fp32 encoding argument overflows: the fp64 oracle's masks differ
    density_only_sees_nothing: bool = False      # the defect sits in the coarse colour head alone
    sized: bool = False                          # `rays` takes a ray count as its second argument

    def make_rays(self, use_view_dirs: bool = True, big: bool = False) -> torch.Tensor:
        """`big`: the BIG_H x BIG_W frame (pinhole cases) or BIG_RAYS rays (ray tables that take a count) of the value tests."""
        if self.rays is not None:
            return self.rays(use_view_dirs, BIG_RAYS) if big and self.sized else self.rays(use_view_dirs)
        h, w = (BIG_H, BIG_W) if big else (H, W)
        fx, fy, cx, cy = O.intrinsics(h, w)
        return O.create_rays(torch.from_numpy(self.pose)[None], h, w, fx, fy, cx, cy, self.near, self.far, use_view_dirs)[0].contiguous()

    def expectation(self, form: str) -> Dict[str, Rays]:
        e = self.expect_novd if form == "no_view_dirs" and self.expect_novd is not None else self.expect
        return {"disp": ACC0, "disp_coarse": ACC0, **e}


def nets(case: Case, D: int, Wd: int, form: str, seed: int = 4100,
         fine_fog: Optional[Tuple[float, float]] = None) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """Thin-fog coarse network and a plain random fine network (tests/test_gpu_accuracy._nets), spoiled as the case says.
    `fine_fog` = (sigma, spread): the fine network's density head is that fog as well (before the spoil), dense enough to end
    rays - the scenes of early termination (tests/mode_domain.py)."""
    novd = form == "no_view_dirs"
    if novd:
        sd_c = synthetic.thin_fog_output(synthetic.make_state_dict(seed + D + Wd, D, Wd, use_view_dirs=False))
        sd_f = synthetic.make_state_dict(seed + 1 + D + Wd, D, Wd, use_view_dirs=False)
    else:
        sd_c = synthetic.thin_fog(synthetic.make_state_dict(seed + D + Wd, D, Wd))
        sd_f = synthetic.make_state_dict(seed + 1 + D + Wd, D, Wd)
    if fine_fog is not None:
        sd_f = (synthetic.thin_fog_output if novd else synthetic.thin_fog)(sd_f, *fine_fog)
    sp = case.spoil_novd if novd and case.spoil_novd is not None else case.spoil
    if sp is not None:
        which, key, idx, value = sp
        sd = sd_c if which == "coarse" else sd_f
        sd[key] = sd[key].copy()
        sd[key][idx] = np.float32(value)
    return sd_c, sd_f


def tensors(sd: Dict[str, np.ndarray]) -> Dict[str, torch.Tensor]:
    return {k: torch.from_numpy(v) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------------------------------
# masks and flags
# ------------------------------------------------------------------------------------------------------------------------

def oracle_key(name: str, fine: bool) -> str:
    """Oracle key of a kernel output; with n_importance == 0 the fine slots receive the coarse results (include/nwe.h)."""
    if name in PER_RAY_FINE:
        return PER_RAY_FINE[name] if fine else PER_RAY_COARSE[name + "_coarse"]
    return {**PER_RAY_COARSE, **PER_SAMPLE, "z_std": "z_std"}[name]


def oracle_masks(res: Dict[str, torch.Tensor], fine: bool) -> Dict[str, np.ndarray]:
    """Element-wise non-finite masks of the oracle outputs under the kernel's output names."""
    out = {}
    for name in OUTPUTS:
        key = oracle_key(name, fine)
        if key in res:
            v = res[key][..., :4] if name in ("raw_coarse", "raw_fine") else res[key]   # use_view_dirs=False: a fifth channel nobody reads
            out[name] = ~torch.isfinite(v).numpy()
    return out


def ray_mask(mask: np.ndarray) -> np.ndarray:
    """[R, ...] element mask -> [R]: the ray has a non-finite element."""
    return mask.reshape(mask.shape[0], -1).any(-1)


def expected_ray_mask(spec: Optional[Rays], n_rays: int, acc: Optional[torch.Tensor] = None) -> np.ndarray:
    """`acc`: the oracle's acc of the pass the output belongs to (for ACC0)."""
    m = np.zeros(n_rays, bool)
    if spec is None:
        return m
    if isinstance(spec, str) and spec == ACC0:
        m[:] = (acc == 0).numpy()
    elif isinstance(spec, str):
        assert spec == ALL, spec
        m[:] = True
    else:
        m[list(spec)] = True
    return m


def expected_flags(res: Dict[str, torch.Tensor], outputs: Sequence[str], fine: bool, density_only: bool = False) -> int:
    """The NWE_FLAG_* word of a render that requested `outputs`, from oracle outputs `res` (include/nwe.h):
      * bits 0-3 / 4-7: rgb, depth, acc, disp of the fine / coarse pass of ANY ray, requested or not (store_ray forms them from
        the composited values, the disparity as 1 / max(1e-10, depth / acc) with a NaN kept); without importance samples both
        groups describe the coarse pass;
      * no NWE_FLAG_RGB_COARSE from a density-only coarse pass (a lean frame of the folded form);
      * NWE_FLAG_RAW only for a requested raw output; NWE_FLAG_ZSTD only when z_std is requested."""
    bad = lambda key: bool((~torch.isfinite(res[key][..., :4] if key.startswith("raw") else res[key])).any())
    word = 0
    side = "fine" if fine else "coarse"
    for bit, name in ((FLAG_RGB, "rgb"), (FLAG_DEPTH, "depth"), (FLAG_ACC, "acc"), (FLAG_DISP, "disp")):
        if bad(f"{name}_{side}"):
            word |= bit
        if bad(f"{name}_coarse") and not (density_only and name == "rgb"):
            word |= bit << 4
    if ("raw_coarse" in outputs and bad("raw_coarse")) or ("raw_fine" in outputs and fine and bad("raw_fine")):
        word |= FLAG_RAW
    if "z_std" in outputs and fine and bad("z_std"):
        word |= FLAG_ZSTD
    return word


# ------------------------------------------------------------------------------------------------------------------------
# rays
# ------------------------------------------------------------------------------------------------------------------------

def _assemble(o: np.ndarray, d: np.ndarray, near, far, use_view_dirs: bool) -> torch.Tensor:
    """[o d near far viewdir] as nerf/rays/rays.py:22-30 forms it (the view direction is d / |d| in fp32)."""
    o, d = torch.from_numpy(np.asarray(o, np.float32)), torch.from_numpy(np.asarray(d, np.float32))
    n = o.shape[0]
    cols = [o, d, torch.as_tensor(near, dtype=torch.float32).expand(n).reshape(n, 1),
            torch.as_tensor(far, dtype=torch.float32).expand(n).reshape(n, 1)]
    if use_view_dirs:
        cols.append(d / torch.norm(d, dim=-1, keepdim=True))
    return torch.cat(cols, 1).contiguous()


def random_rays(n: int, seed: int, origin_scale: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """Origins uniform in [-1, 1]^3 times `origin_scale`, random directions of length 0.5 .. 2."""
    rng = np.random.Generator(np.random.Philox(key=[seed, n]))
    o = (rng.uniform(-1.0, 1.0, (n, 3)) * origin_scale).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    return o, d


SWEEP_SCALES = (0.0, 1e-20, 1.0, 22.0, 1e2, 1e3, 1e4, 4e5)      # inside the documented range of every mode (|x| < 5e5)
SWEEP_BEYOND = (1e6, 3e7, 1e12)                                 # beyond it: the criterion, or NaN with the flags raised
SWEEP_OVERFLOW = 3e38                                           # x / 10 * 2^9 overflows fp32: sin(inf) = NaN in the reference
SWEEP_RAYS = 32


def sweep_rays(scale: float, use_view_dirs: bool = True, n: int = SWEEP_RAYS) -> torch.Tensor:
    o, d = random_rays(n, 77, scale)
    if scale >= 1.0:                 # every coordinate of magnitude `scale`, not just below it
        o = (np.sign(o) * np.float32(scale) * (0.5 + 0.5 * np.abs(o) / np.float32(max(scale, 1e-30)))).astype(np.float32)
    return _assemble(o, d, NEAR, FAR, use_view_dirs)


POISON = {3: "nan_origin", 17: "inf_origin", 20: "zero_dir", 31: "nan_dir", 32: "far_inf", 45: "underflow_dir", 63: "nan_near"}
POISON_RAYS = 70                     # three packets of 32, the last one ragged


def poisoned_rays(use_view_dirs: bool = True, n: int = POISON_RAYS, healthy_only: bool = False) -> torch.Tensor:
    """n (70) healthy rays; unless `healthy_only`, the rays of POISON are spoiled in place (their neighbours are untouched)."""
    o, d = random_rays(n, 78)
    near, far = np.full(n, NEAR, np.float32), np.full(n, FAR, np.float32)
    if not healthy_only:
        for i, kind in POISON.items():
            if kind == "nan_origin":
                o[i, 1] = np.nan
            elif kind == "inf_origin":
                o[i, 0] = np.inf
            elif kind == "zero_dir":
                d[i] = 0.0
            elif kind == "nan_dir":
                d[i, 2] = np.nan
            elif kind == "far_inf":
                far[i] = np.inf
            elif kind == "underflow_dir":
                d[i] = d[i] * np.float32(1e-30)
            elif kind == "nan_near":
                near[i] = np.nan
    with np.errstate(all="ignore"):
        return _assemble(o, d, near, far, use_view_dirs)


def _scaled_rotation(scale: float) -> np.ndarray:
    p = _pose()
    p[:3, :3] *= np.float32(scale)
    return p


def _nan_pose() -> np.ndarray:
    p = _pose()
    p[1, 0] = np.nan                 # one rotation entry: the y component of every direction
    return p


# ------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------

_VIEW = ("rgb", "rgb_coarse", "raw_coarse", "raw_fine")                       # what a NaN view direction reaches
_EVERYTHING = {k: ALL for k in OUTPUTS}
_NO_ACC = {"disp": ALL, "disp_coarse": ALL}                                   # acc = 0 on every ray
_zero_dir = {**{k: ALL for k in _VIEW}, **_NO_ACC}
_poison_all = [i for i, k in POISON.items() if k in ("nan_origin", "inf_origin", "nan_dir", "far_inf", "nan_near")]
_poison_view = [i for i, k in POISON.items() if k in ("zero_dir", "underflow_dir")]
_poisoned = {k: sorted(_poison_all + (_poison_view if k in _VIEW + tuple(_NO_ACC) else [])) for k in OUTPUTS}
_poisoned_novd = {k: sorted(_poison_all + (_poison_view if k in _NO_ACC else [])) for k in OUTPUTS}
# (the healthy rays of that table all meet density: asserted by the CPU test through the explicit disp lists)

CASES: List[Case] = [
    # -- geometry ----------------------------------------------------------------------------------------------------------
    Case("healthy", {}, pose=_pose(), values=True),
    # every depth equal: all distances 0 but the last, whose alpha is 1 - exp(-relu(sigma) 1e10 |d|)
    # (1 where sigma > 0 there, else 0: acc is 0 or 1 and the disparity NaN where it is 0)
    Case("near_eq_far", {}, pose=_pose(), near=2.0, far=2.0, values=True),
    # a zero rotation: d = 0, the view direction 0 / 0; every point is the origin, every distance 0, acc = 0
    Case("zero_direction", _zero_dir, pose=_scaled_rotation(0.0), expect_novd=_NO_ACC),
    # |d| ~ 1e-30: its fp32 norm underflows to 0 and the view direction is d / 0 = inf, gamma(d) = sin(inf) = NaN
    Case("underflow_direction", _zero_dir, pose=_scaled_rotation(1e-30), expect_novd=_NO_ACC),
    # z = near (1 - t) + inf t: NaN at t = 0, inf behind it
    Case("far_inf", _EVERYTHING, pose=_pose(), far=float("inf")),
    # NaN directions: every point; the coarse depths (and the z_fine entries they fill) stay finite, the samples drawn from NaN weights do not
    Case("nan_c2w", _EVERYTHING, pose=_nan_pose()),
    Case("poisoned_neighbours", _poisoned, rays=poisoned_rays, sized=True, expect_novd=_poisoned_novd),
    # -- networks ----------------------------------------------------------------------------------------------------------
    Case("nan_weight_coarse_trunk", _EVERYTHING, pose=_pose(), spoil=("coarse", "_pts_linears.2.weight", (5, 7), np.nan)),
    Case("nan_weight_fine_trunk", {k: ALL for k in ("rgb", "depth", "acc", "disp", "raw_fine")}, pose=_pose(),
         spoil=("fine", "_pts_linears.2.weight", (5, 7), np.nan)),
    Case("inf_weight_coarse_trunk", _EVERYTHING, pose=_pose(), spoil=("coarse", "_pts_linears.1.weight", (5, 7), np.inf)),
    Case("inf_weight_fine_trunk", {k: ALL for k in ("rgb", "depth", "acc", "disp", "raw_fine")}, pose=_pose(),
         spoil=("fine", "_pts_linears.1.weight", (9, 11), np.inf)),
    Case("nan_bias_fine_trunk", {k: ALL for k in ("rgb", "depth", "acc", "disp", "raw_fine")}, pose=_pose(),
         spoil=("fine", "_pts_linears.1.bias", (4,), np.nan)),
    Case("nan_bias_coarse_trunk", _EVERYTHING, pose=_pose(), spoil=("coarse", "_pts_linears.3.bias", (100,), np.nan)),
    # sigma alone is NaN: the weights, so every composited value and the samples drawn from them
    Case("nan_alpha_linear_coarse", _EVERYTHING, pose=_pose(), spoil=("coarse", "_alpha_linear.weight", (0, 9), np.nan),
         spoil_novd=("coarse", "_output_linear.weight", (3, 9), np.nan)),
    Case("nan_alpha_linear_fine", {k: ALL for k in ("rgb", "depth", "acc", "disp", "raw_fine")}, pose=_pose(),
         spoil=("fine", "_alpha_linear.weight", (0, 9), np.nan), spoil_novd=("fine", "_output_linear.weight", (3, 9), np.nan)),
    # colour alone: depth and acc of that pass are untouched; a density-only coarse pass never evaluates the coarse colour
    Case("nan_rgb_linear_coarse", {"rgb_coarse": ALL, "raw_coarse": ALL}, pose=_pose(), density_only_sees_nothing=True,
         spoil=("coarse", "_rgb_linear.weight", (1, 3), np.nan), spoil_novd=("coarse", "_output_linear.weight", (1, 3), np.nan)),
    Case("nan_rgb_linear_fine", {"rgb": ALL, "raw_fine": ALL}, pose=_pose(),
         spoil=("fine", "_rgb_linear.weight", (1, 3), np.nan), spoil_novd=("fine", "_output_linear.weight", (1, 3), np.nan)),
]
# -- coordinate sweep: every output finite in the reference up to 1e12; at 3e38 the fp32 product x / 10 * 2^9 is inf ----------
for _s in SWEEP_SCALES + SWEEP_BEYOND:
    CASES.append(Case(f"origin_{_s:g}", {}, rays=(lambda vd, s=_s: sweep_rays(s, vd))))
CASES.append(Case(f"origin_{SWEEP_OVERFLOW:g}", _EVERYTHING, rays=(lambda vd: sweep_rays(SWEEP_OVERFLOW, vd)), f32_overflow=True))

BY_NAME = {c.name: c for c in CASES}
NETWORK_CASES = [c.name for c in CASES if c.spoil is not None]
GEOMETRY_CASES = ["near_eq_far", "zero_direction", "underflow_direction", "far_inf", "nan_c2w"]
SWEEP_CASES = [c.name for c in CASES if c.name.startswith("origin_")]

# shapes the GPU test instantiates: 8x256 and 4x128 folded, one without view directions, one in the reference formulation
INSTANTIATIONS = [(8, 256, "folded"), (4, 128, "folded"), (8, 256, "no_view_dirs"), (4, 128, "reference")]
NS, NI = 64, 128


def run_oracle(case: Case, D: int, Wd: int, form: str, dtype: torch.dtype = torch.float32, ns: int = NS, ni: int = NI,
               big: bool = False, fine_fog: Optional[Tuple[float, float]] = None):
    """(rays, coarse state, fine state, oracle outputs) of a case in `dtype`."""
    sd_c, sd_f = nets(case, D, Wd, form, fine_fog=fine_fog)
    rays = case.make_rays(form != "no_view_dirs", big)
    res = O.render_rays(rays, tensors(sd_c), tensors(sd_f) if ni else None, O.RenderConfig(n_samples=ns, n_importance=ni), dtype=dtype)
    return rays, sd_c, sd_f, res
