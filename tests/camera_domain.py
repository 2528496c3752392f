"""The legal camera domain of nwe_render / nwe_create_rays / nwe_render_tiled: one table of named cases shared by
tests/test_camera_domain_oracle.py (CPU) and tests/test_camera_domain_gpu.py (GPU), like tests/shape_domain.py and
tests/input_domain.py are shared by theirs.  Plain data plus helpers; nothing here touches a GPU.

A case gives a frame (H, W), the four intrinsics as the ABI takes them (independent floats), a [B,4,4] fp32 pose array, an
optional row window and the depth bounds.  Every case produces finite, non-zero rays: zero directions, NaN poses and non-finite
bounds are tests/input_domain.py's.  The frames are tiny (at most 400 rays) so that tests/golden/cameras.npz can hold every ray
of every case; `hybrid_case` alone is large, sized from the CU count, and is compared against the live oracle.

Every pose is made of literals and of IEEE +, -, *, /, sqrt in fp64, rounded to fp32 once: the same bits on every machine.

`restated_rays` is the arithmetic nwe_device.h documents for seed_ray / make_ray / norm3, in numpy: what the kernels must
compute.  Its `twin` argument gives the WRONG variants (TWINS) the table is there to tell from the truth; each case names in
`catches` the twins it must distinguish, and tests/test_camera_domain_oracle.py holds the table to that on the CPU.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import nerf_oracle as O

F = np.float32
MAX_GOLDEN_RAYS = 400                            # per case: the golden file holds every ray of every case of CASES

# the wrong variants of ray generation a case may have to tell from the truth (restated_rays)
TWINS = ("swap_f",          # fx and fy exchanged anywhere in the argument chain
         "swap_c",          # cx and cy exchanged
         "fma",             # make_ray's products contracted: fma(m1, y, m0 * x) + m2
         "rcp",             # (w - cx) * (1 / fx) for the true division
         "no_row_begin",    # the row window's first row dropped: h counted from 0
         "row3",            # row 3 of c2w read as a translation
         "transpose",       # the 3x3 part read column-major
         "no_zero_start")   # the three products summed without torch's +0 accumulator: products that are all -0 sum to -0

# the kinds of case the table must contain (tests/test_camera_domain_oracle.py::test_table_covers_every_kind)
KINDS = ("control", "focal-square", "focal-nonsquare", "neg-fx", "neg-fy", "neg-both", "pp-offcentre", "pp-integer-posfx",
         "pp-integer-negfx", "pp-outside-low", "pp-outside-high", "inexact-quotient", "telephoto", "wide", "frame-1x1",
         "frame-1xW", "frame-Hx1", "frame-wide-row", "batch-window", "general-linear", "general-shear", "axis-aligned",
         "garbage-row3", "large-translation")


@dataclass(frozen=True)
class Case:
    name: str
    kind: str
    H: int
    W: int
    fx: float
    fy: float
    cx: float
    cy: float
    poses: np.ndarray                            # [B,4,4] fp32
    rows: Optional[Tuple[int, int]] = None       # row window [begin, end), None = the whole frame
    near: float = 0.1
    far: float = 10.0
    catches: Tuple[str, ...] = ()                # twins whose rays must differ in bits from this case's
    tiled: bool = False                          # also rendered by three contexts (nwe_render_tiled)

    @property
    def window(self) -> Tuple[int, int]:
        return self.rows if self.rows is not None else (0, self.H)

    @property
    def n_poses(self) -> int:
        return int(self.poses.shape[0])

    @property
    def n_rays(self) -> int:
        r0, r1 = self.window
        return self.n_poses * (r1 - r0) * self.W

    @property
    def intrinsics(self) -> Dict[str, float]:
        return dict(fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy)

    def camera(self) -> Dict[str, float]:
        """The keyword arguments of Renderer.render / create_rays that describe the camera."""
        return dict(fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy, near=self.near, far=self.far)


# ------------------------------------------------------------------------------------------------------------------------
# poses
# ------------------------------------------------------------------------------------------------------------------------

def _pose(rot3x3, t, bottom=(0.0, 0.0, 0.0, 1.0)) -> np.ndarray:
    m = np.zeros((4, 4), dtype=np.float64)
    m[:3, :3] = np.asarray(rot3x3, dtype=np.float64)
    m[:3, 3] = t
    m[3] = bottom
    return m.astype(F)


def _quat_rot(w: float, x: float, y: float, z: float) -> np.ndarray:
    """Rotation matrix of the quaternion (w, x, y, z) / |(w, x, y, z)|, fp64, written out entry by entry."""
    n = np.sqrt(np.float64(w * w + x * x + y * y + z * z))
    w, x, y, z = (np.float64(v) / n for v in (w, x, y, z))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def _rigid(q: Sequence[float], t: Sequence[float]) -> np.ndarray:
    return _pose(_quat_rot(*q), t)


T0 = (0.0, -0.5, -0.76)                                         # inside the synthetic scene, as the other GPU tests' poses
Q_CONTROL = (0.61, 0.35, -0.58, 0.41)                           # every entry of the rotation is far from 0 and from +-1
# far from symmetric: |R - R^T| ~ 1, so that rows and columns cannot be mixed up unnoticed
Q_SKEW = (0.31, -0.77, 0.22, 0.51)
POSE_CONTROL = _rigid(Q_CONTROL, T0)[None]
POSE_SKEW = _rigid(Q_SKEW, (0.3, -0.45, -0.9))[None]

# five mutually different poses
POSES_BATCH = np.stack([_rigid((0.9, 0.1, 0.4, -0.2), (0.1, -0.5, -0.7)), _rigid((0.2, 0.8, -0.3, 0.5), (-0.2, -0.4, -0.8)),
                        _rigid((-0.4, 0.3, 0.7, 0.6), (0.3, -0.6, -0.6)), _rigid((0.5, -0.5, 0.6, 0.1), (0.0, -0.3, -0.9)),
                        _rigid((0.7, 0.6, 0.2, -0.3), (-0.1, -0.55, -0.75))])

# nine distinct entries of mixed sign and scale; column norms 0.01, 1 and 30 (unit columns scaled)
_COLS = np.array([[0.48, -0.6, 0.64], [-0.36, 0.48, 0.8], [0.8, 0.6, 0.0]], dtype=np.float64).T     # columns: unit vectors
_COLS[:, 2] = (0.28, -0.6, 0.752)                                                                    # third: no zero entry, norm ~1
GENERAL = _COLS * np.array([0.01, 1.0, 30.0])
SHEAR = np.array([[1.0, 0.75, -0.4], [0.0, 1.0, 1.3], [0.0, 0.0, 1.0]])
POSE_GENERAL = _pose(GENERAL, (0.2, -0.5, -0.7))[None]
POSE_SHEAR = _pose(GENERAL @ SHEAR, (0.2, -0.5, -0.7))[None]

# 90-degree steps: entries +-1 and +-0.0, the negative zero included; none of the four is symmetric or the identity
POSES_AXIS = np.stack([_pose([[0.0, -1.0, -0.0], [0.0, 0.0, -1.0], [1.0, -0.0, 0.0]], T0),
                       _pose([[-0.0, 0.0, 1.0], [-1.0, 0.0, -0.0], [0.0, -1.0, 0.0]], T0),
                       _pose([[0.0, 1.0, 0.0], [-1.0, -0.0, 0.0], [-0.0, 0.0, 1.0]], T0),
                       _pose([[-1.0, 0.0, -0.0], [0.0, -0.0, 1.0], [0.0, 1.0, 0.0]], T0)])

POSE_ROW3_CLEAN = _rigid(Q_SKEW, (0.25, -0.5, -0.8))[None]
POSE_ROW3_GARBAGE = _pose(_quat_rot(*Q_SKEW), (0.25, -0.5, -0.8), bottom=(7.0, 8.0, 9.0, 10.0))[None]
POSE_FAR_AWAY = _rigid(Q_CONTROL, (1e4, -1e4, 1e4))[None]

F400 = 400.0 * (1.0 + 2.0 ** -20)


def _c90(H: int, W: int) -> Dict[str, float]:
    fx, fy, cx, cy = O.intrinsics(H, W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy)


ANY = ("fma", "transpose")                      # what every general rotation with inexact products tells apart

CASES: List[Case] = [
    # the 90-degree family every other GPU test uses: fx == fy, the principal point at the grid centre
    Case("control-12x16", "control", 12, 16, **_c90(12, 16), poses=POSE_CONTROL, catches=ANY),
    # fx != fy.  On the square frame with cx == cy only the focal lengths can be told apart; H = 13 and 10: tiles of 5 + 4 + 4
    # and 4 + 3 + 3 rows
    Case("focal-square-13x13", "focal-square", 13, 13, 37.3, 91.7, 6.0, 6.0, POSE_SKEW, catches=("swap_f",) + ANY, tiled=True),
    Case("focal-10x14", "focal-nonsquare", 10, 14, 37.3, 91.7, 6.5, 4.5, POSE_CONTROL, catches=("swap_f", "swap_c", "transpose"), tiled=True),
    # negative focal lengths mirror
    Case("neg-fx", "neg-fx", 9, 11, -41.3, 41.3, 5.0, 4.0, POSE_SKEW, catches=("swap_f",)),
    Case("neg-fy", "neg-fy", 9, 11, 41.3, -41.3, 5.0, 4.0, POSE_SKEW, catches=("swap_f",)),
    Case("neg-both", "neg-both", 9, 11, -41.3, -29.9, 5.0, 4.0, POSE_CONTROL, catches=("swap_f",)),
    # principal point off the centre, not on a pixel; fx == fy, so only cx / cy can be told apart; tiles of 5 + 5 + 4 rows
    Case("pp-offcentre-14x12", "pp-offcentre", 14, 12, 23.0, 23.0, 3.37, 10.81, POSE_SKEW, catches=("swap_c",), tiled=True),
    # principal point ON a pixel: (w - cx) is exactly +0 there, and with fx < 0 x = -0
    Case("pp-integer-posfx", "pp-integer-posfx", 8, 12, 17.0, 19.0, 5.0, 3.0, POSE_SKEW, catches=("swap_c",)),
    Case("pp-integer-negfx", "pp-integer-negfx", 8, 12, -17.0, 19.0, 5.0, 3.0, POSE_SKEW, catches=("swap_c", "swap_f")),
    # principal point outside the image, either side
    Case("pp-outside-low", "pp-outside-low", 8, 10, 31.0, 27.0, -20.5, 20.0, POSE_CONTROL, catches=("swap_c",)),
    Case("pp-outside-high", "pp-outside-high", 8, 10, 31.0, 27.0, 20.25, -7.75, POSE_SKEW, catches=("swap_c",)),
    # quotients that are inexact, and differ from a multiplication by the reciprocal
    Case("inexact-3-7", "inexact-quotient", 12, 16, 3.0, 7.0, 7.5, 5.5, POSE_CONTROL, catches=("rcp", "swap_f")),
    Case("inexact-400eps", "inexact-quotient", 12, 16, F400, 3.0, 7.5, 5.5, POSE_SKEW, catches=("rcp",)),
    # extreme focal lengths
    Case("telephoto-1e5", "telephoto", 12, 16, 1e5, 1e5, 7.5, 5.5, POSE_SKEW, catches=("transpose",)),
    Case("wide-0.05", "wide", 12, 16, 0.05, 0.05, 7.5, 5.5, POSE_CONTROL, catches=ANY),
    # frame-shape edges
    Case("frame-1x1", "frame-1x1", 1, 1, 1.5, 2.5, 0.25, -0.5, POSE_SKEW, near=0.05, far=6.0, catches=("swap_f", "swap_c")),
    Case("frame-1x37", "frame-1xW", 1, 37, 21.0, 33.0, 17.3, 0.4, POSE_CONTROL, catches=("swap_f", "swap_c")),
    Case("frame-37x1", "frame-Hx1", 37, 1, 21.0, 33.0, 0.4, 17.3, POSE_CONTROL, catches=("swap_f", "swap_c")),
    Case("frame-3x129", "frame-wide-row", 3, 129, 70.0, 50.0, 63.1, 1.2, POSE_SKEW, catches=("swap_f", "swap_c")),
    # five poses, a row window that touches neither end; H = 11: tiles of 4 + 4 + 3 rows
    Case("batch5-rows3to9-11x7", "batch-window", 11, 7, 9.5, 6.25, 2.75, 5.5, POSES_BATCH, rows=(3, 9), near=0.2, far=8.0,
         catches=("no_row_begin", "swap_f", "swap_c") + ANY, tiled=True),
    # a general linear map instead of a rotation, and the same with a shear
    Case("general-linear", "general-linear", 10, 12, 14.0, 11.0, 5.2, 4.9, POSE_GENERAL, catches=("transpose", "swap_f")),
    Case("general-shear", "general-shear", 10, 12, 14.0, 11.0, 5.2, 4.9, POSE_SHEAR, catches=("transpose", "swap_f")),
    # products with zero entries of either sign: where all three are -0 the reference's sum is +0 (its accumulator starts at +0)
    Case("axis-aligned", "axis-aligned", 5, 6, 4.0, 8.0, 2.0, 3.0, POSES_AXIS, catches=("transpose", "swap_f", "swap_c", "no_zero_start")),
    # row 3 of c2w is not read: (7, 8, 9, 10) there changes nothing against the clean twin below
    Case("row3-garbage", "garbage-row3", 9, 10, 12.5, 10.5, 4.1, 4.6, POSE_ROW3_GARBAGE, catches=("row3",)),
    Case("row3-clean", "garbage-row3", 9, 10, 12.5, 10.5, 4.1, 4.6, POSE_ROW3_CLEAN),
    Case("translation-1e4", "large-translation", 8, 10, 13.0, 11.0, 4.5, 3.5, POSE_FAR_AWAY, catches=ANY),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
CONTROL = CASES[0]
TILED_NAMES = [c.name for c in CASES if c.tiled]
GARBAGE_PAIR = ("row3-garbage", "row3-clean")

RAYS_PER_WORKGROUP = 128                         # csrc/nwe_mfma_config.h: four packets of 32 rays


def hybrid_case(cus: int) -> Case:
    """Three poses, a row window, intrinsics off the centre, sized so that the ray count exceeds one round of packet workgroups
    (cus x 128 rays) by less than a round: under the hybrid plan the second launch then starts at ray cus x 128, inside a row of
    the last pose.  256 CUs: rows (10, 110) of 120 x 111 columns x 3 poses = 33 300 rays, 532 more than the round."""
    first = cus * RAYS_PER_WORKGROUP
    for W, extra in ((111, 2), (111, 1), (113, 2), (113, 1), (109, 2), (109, 1)):
        rows = first // (3 * W) + extra
        rest = first - 2 * rows * W              # ray_first within the last pose
        if 0 < rest < rows * W and rest % W != 0:
            return Case(f"hybrid-{cus}cu", "hybrid", rows + 20, W, 61.7, 84.3, 40.6, 71.9, POSES_BATCH[1:4], rows=(10, 10 + rows),
                        catches=("no_row_begin", "swap_f", "swap_c"))
    raise ValueError(f"no hybrid frame for {cus} CUs")


# ------------------------------------------------------------------------------------------------------------------------
# rays
# ------------------------------------------------------------------------------------------------------------------------

def window_of(full: np.ndarray, case: Case) -> np.ndarray:
    """[B, H*W, C] rays of whole frames -> [B*rows*W, C], the rays of the case's row window in the ABI's order."""
    r0, r1 = case.window
    B, _, C = full.shape
    return np.ascontiguousarray(full.reshape(B, case.H, case.W, C)[:, r0:r1].reshape(-1, C))


def oracle_frames(case: Case, use_view_dirs: bool = True) -> np.ndarray:
    """The oracle's create_rays on the whole frames: [B, H*W, 11 | 8]."""
    return O.create_rays(torch.from_numpy(case.poses), case.H, case.W, case.fx, case.fy, case.cx, case.cy, case.near, case.far,
                         use_view_dirs).numpy()


def oracle_rays(case: Case, use_view_dirs: bool = True) -> np.ndarray:
    return window_of(oracle_frames(case, use_view_dirs), case)


def bits(a) -> np.ndarray:
    """fp32 -> int32 view: comparisons through it tell +0 from -0 (and any NaN payloads apart)."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.int32)


def same_bits(a, b) -> bool:
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def fma32(a, b, c) -> np.ndarray:
    """fp32 fma(a, b, c), correctly rounded: the product of two fp32 numbers is exact in fp64; the fp64 sum is rounded TO ODD
    (its exact error comes from the two-sum) so that the second rounding, to fp32, cannot go wrong."""
    a, b, c = (np.asarray(v, dtype=F) for v in (a, b, c))
    p, c64 = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    even = (s.view(np.int64) & 1) == 0 if s.ndim else (np.array(s).view(np.int64) & 1) == 0
    odd = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return odd.astype(F)


def restated_rays(case: Case, twin: Optional[str] = None, use_view_dirs: bool = True) -> np.ndarray:
    """[B*rows*W, 11 | 8]: the arithmetic csrc/nwe_device.h documents, every operation in fp32, one rounding each.

        x = (w - cx) / fx,  y = (h - cy) / fy                       true divisions (seed_ray)
        d_i = ((0 + m[i][0] * x) + m[i][1] * y) + m[i][2]           products rounded, summed left to right onto +0 as torch's
                                                                    matmul accumulates them, no FMA (make_ray): -0 only from x + -x
        o = (m[0][3], m[1][3], m[2][3]);  row 3 of m is not read
        |d| = sqrt(fma(dz, dz, fma(dy, dy, dx * dx)))               (norm3), correctly rounded sqrt
        v = d / |d|                                                 true divisions

    `twin`: one of TWINS, the same with that one mistake."""
    assert twin is None or twin in TWINS, twin
    fx, fy, cx, cy = (F(v) for v in (case.fx, case.fy, case.cx, case.cy))
    if twin == "swap_f":
        fx, fy = fy, fx
    if twin == "swap_c":
        cx, cy = cy, cx
    r0, r1 = case.window
    w = np.arange(case.W, dtype=F)
    h = np.arange(0 if twin == "no_row_begin" else r0, (r1 - r0) if twin == "no_row_begin" else r1, dtype=F)
    if twin == "rcp":
        x, y = (w - cx) * (F(1) / fx), (h - cy) * (F(1) / fy)
    else:
        x, y = (w - cx) / fx, (h - cy) / fy
    X = np.broadcast_to(x[None, :], (h.size, w.size)).reshape(-1)
    Y = np.broadcast_to(y[:, None], (h.size, w.size)).reshape(-1)
    out = []
    for m in case.poses:
        R = m[:3, :3].T if twin == "transpose" else m[:3, :3]
        if twin == "fma":
            d = [fma32(R[i, 1], Y, fma32(R[i, 0], X, F(0))) + R[i, 2] for i in range(3)]
        elif twin == "no_zero_start":
            d = [(R[i, 0] * X + R[i, 1] * Y) + R[i, 2] for i in range(3)]
        else:
            d = [((F(0) + R[i, 0] * X) + R[i, 1] * Y) + R[i, 2] for i in range(3)]
        o = m[:3, 3] + m[3, :3] if twin == "row3" else m[:3, 3]
        cols = [np.full_like(X, o[i]) for i in range(3)] + d + [np.full_like(X, F(case.near)), np.full_like(X, F(case.far))]
        if use_view_dirs:
            n = np.sqrt(fma32(d[2], d[2], fma32(d[1], d[1], d[0] * d[0])))
            cols += [d[i] / n for i in range(3)]
        out.append(np.stack(cols, axis=-1))
    res = np.concatenate(out, axis=0)
    assert res.dtype == F
    return res
