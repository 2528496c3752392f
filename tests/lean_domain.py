"""The lean pinhole frame - rgb / depth / acc only, the call of the GUI and the benchmark - in every shape it is built for: the
LEAN instantiations with the density-only coarse pass and the hollow colour path, the work queue, the tail kernel
(csrc/nwe_mfma_render.h: render_mfma_tail_kernel) and packets of 8x4 pixel blocks, all at once.  The shape list, the frames,
the judged rays, the scenes and the CPU oracles shared by tests/test_lean_domain_host.py (CPU) and tests/test_gpu_lean_domain.py
(GPU).  Nothing here needs a GPU.

Every frame is made by rule from the device's CU count: g(n) is the grid of a queued launch of n items, surplus = g(cus) - cus
the workgroups a queued round of packets starts beyond its items, and a frame of cus * 128 + k * 32 rays (the last item may
be ragged) is one round of packets plus k sample-split items, which the packets launch renders in its tail exactly if
k <= surplus (csrc/nwe_plan.cpp)."""
import functools

import numpy as np
import torch

from oracle import nerf_oracle as O
from tests import mode_domain as M
from tests.test_gpu_work_queue_tail import _hw

# ---- shapes ---------------------------------------------------------------------------------------------------------------------
# every (D, W, form) csrc/nwe_mfma_shapes.h lists, in the order of tests/test_gpu_accuracy.INSTANTIATIONS;
# tests/test_lean_domain_host.py holds the list to both
FOLDED = [(8, 256), (4, 128), (8, 128), (4, 256), (6, 256), (6, 128)]
REFERENCE = [(8, 256), (4, 128)]
NO_VIEW_DIRS = [(8, 256), (4, 128), (6, 256), (4, 256), (8, 128), (6, 128)]
SHAPES = ([(D, W, "folded") for D, W in FOLDED] + [(D, W, "reference") for D, W in REFERENCE] +
          [(D, W, "no_view_dirs") for D, W in NO_VIEW_DIRS])
FORM_TOKENS = {"kFormFolded": "folded", "kFormReference": "reference", "kFormNoViewDirs": "no_view_dirs"}   # nwe_mfma_shapes.h


def kind(D, W, form):
    """'6x128', '6x128-noview', '4x128-reference'."""
    return f"{D}x{W}" + {"folded": "", "reference": "-reference", "no_view_dirs": "-noview"}[form]


IDS = [kind(*s) for s in SHAPES]
PRECISIONS = ("f16x3", "f16x1")
LEAN = ("rgb", "depth", "acc")
FULL = LEAN + ("rgb_coarse",)             # one output more: the FULL instantiation - never queued onto the tail, never blocked
NEAR, FAR = 0.1, 10.0

# (n_samples, n_importance) -> white background.  13 + 9: both passes ragged against the sample-split plan's four samples per
# iteration, a density-only coarse pass where that is built (the 6-deep shapes keep the coarse colour); 7 + 0: the coarse pass
# is the frame, no density-only pass runs.  64 + 128 once per formulation.
SAMPLINGS = {(13, 9): True, (7, 0): False}
LONG = (64, 128)
LONG_SHAPES = [(8, 256, "folded"), (6, 128, "folded"), (4, 128, "no_view_dirs")]
WHITE = {**SAMPLINGS, LONG: False}


def samplings(D, W, form):
    return list(SAMPLINGS) + ([LONG] if (D, W, form) in LONG_SHAPES else [])


def density_only(D, W, form):
    """M.density_only with the reference formulation, which has the density-only coarse pass of the folded one."""
    return form != "no_view_dirs" and D != 6


def fold(form):
    """debug_set_fold of a formulation: the reference formulation is the folded state dict packed unfolded."""
    return form != "reference"


def nets(D, W, form):
    """M.fog_nets(.., 'thin'): networks 1000 / 1001 of the shape with a thin fog in both density heads; the reference
    formulation takes the folded ones.  (The plain random fine network of tests/test_gpu_accuracy._nets gives a mean acc of
    0.001 at 4x128 without view directions: too empty to notice a colour error.)"""
    return M.fog_nets(D, W, "folded" if form == "reference" else form, "thin")


# ---- frames by rule from cus ----------------------------------------------------------------------------------------------------

def grid(n):
    """The grid of a queued launch of n items (csrc/nwe_plan.h: queue_grid)."""
    return (n + (n + 3) // 4 + 7) // 8 * 8


def surplus(cus):
    return grid(cus) - cus


def _ragged_rays(cus, k):
    return cus * 128 + (k - 1) * 32 + 5


def ragged(cus):
    """(k, H, W): one round of packets plus k split items, the last 5 rays wide; k the largest value up to the surplus whose ray
    count is an H x W product with both sides below 8192.  The width is no multiple of 8: packet blocks cannot apply."""
    for k in range(surplus(cus), 0, -1):
        hw = _hw(_ragged_rays(cus, k))
        if hw:
            return (k,) + hw
    raise ValueError(f"no ragged frame at {cus} CUs")


def one_past(cus):
    """(k, H, W) of the ragged frame's rule with k = surplus + 1 (the next k whose ray count is a product, should that one not
    be): one split item more than the surplus covers, the path must not be taken."""
    for k in range(surplus(cus) + 1, 2 * surplus(cus) + 64):
        hw = _hw(_ragged_rays(cus, k))
        if hw:
            return (k,) + hw
    raise ValueError(f"no frame one past the surplus at {cus} CUs")


def _blocked_hw(n):
    """(H, W) with H * W == n, H a multiple of 4 and W of 8, the two nearest to each other (H <= W on a tie); None if none."""
    best = None
    for h in range(4, min(n // 8, 8191) + 1, 4):
        if n % h == 0 and (n // h) % 8 == 0 and n // h < 8192:
            if best is None or (abs(h - n // h), h) < (abs(best[0] - best[1]), best[0]):
                best = (h, n // h)
    return best


def blocked(cus):
    """(k, H, W): H % 4 == 0, W % 8 == 0 and H * W = cus * 128 + k * 32 with 1 <= k <= surplus; of these the k nearest to a
    quarter of the surplus (the smaller on a tie) - away from both ends of the condition, which the ragged frame and the one
    past it hold - and the frame nearest to square.  160 x 208 with k = 16 at 256 CUs."""
    s = surplus(cus)
    for k in sorted(range(1, s + 1), key=lambda k: (abs(k - s // 4), k)):
        hw = _blocked_hw(cus * 128 + k * 32)
        if hw:
            return (k,) + hw
    raise ValueError(f"no blocked frame at {cus} CUs")


SMALL = (13, 29, 3)                        # H, W, poses: 1131 rays, no tail; the queue under plans 0 / 1 / 2
SMALL_RAYS = SMALL[0] * SMALL[1] * SMALL[2]


def pose(yaw=-30.0):
    return O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, yaw, 0.0, 0.0))[0].numpy()


SMALL_POSES = np.stack([pose(), pose(-75.0), pose(10.0)])


def camera(H, W):
    fx, fy, cx, cy = O.intrinsics(H, W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR)


def hollow_frame(cus, width=800, centre=400):
    """(k, (row0, row1)) of the hollow test on the 800-wide frame of tests/hollow_domain.py: width * rows = cus * 128 + k * 32
    with 1 <= k <= surplus, the largest such row count (most split items), about the rows of that module's scene; None if there
    is none.  43 rows, [379, 422), and k = 51 at 256 CUs (43 is no multiple of 4: the frame stays linear)."""
    for rows in range((cus * 128 + surplus(cus) * 32) // width, 0, -1):
        extra = width * rows - cus * 128
        if extra <= 0:
            break
        if extra % 32 == 0 and rows < 2 * centre:
            return extra // 32, (centre - rows // 2, centre - rows // 2 + rows)
    return None


# ---- judged rays ----------------------------------------------------------------------------------------------------------------

def judged(cus, n_rays):
    """Ray indices of a ragged frame held to the oracles: the first 128 (packet item 0), the last packets item and the first
    two split items (cus * 128 - 128 .. cus * 128 + 63), and the last 69 (the ragged item and the two in front of it)."""
    idx = np.concatenate([np.arange(128), np.arange(cus * 128 - 128, cus * 128 + 64), np.arange(n_rays - 69, n_rays)])
    assert idx.min() >= 0 and idx.max() == n_rays - 1
    return np.unique(idx)


def _tensors(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def frame_rays(cus, view=True):
    """(k, H, W, judged indices, their oracle rays [389, 11 | 8]) of the ragged frame; shared: leave it unchanged."""
    k, H, W = ragged(cus)
    cam = camera(H, W)
    rays = O.create_rays(torch.from_numpy(pose())[None], H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], NEAR, FAR, view)[0]
    idx = judged(cus, H * W)
    return k, H, W, idx, rays[torch.from_numpy(idx)].contiguous()


@functools.lru_cache(maxsize=None)
def oracles(cus, D, W, form, sampling):
    """(ref32, ref64, keep) on the judged rays of the ragged frame: the fp32 and the fp64 oracle's rgb / depth / acc under the
    sampling's white background, and the project's own rule for the rays compared (tests/test_gpu_accuracy.e2e_accuracy: the
    last sample's |sigma| >= 1e-5 in fp64 - below it the ray sits on the alpha step of the 1e10 interval).  Shared."""
    ns, ni = sampling
    sd_c, sd_f = nets(D, W, form)
    rays = frame_rays(cus, form != "no_view_dirs")[4]
    cfg = O.RenderConfig(n_samples=ns, n_importance=ni, white_bkgd=WHITE[sampling])
    tc, tf = _tensors(sd_c), (_tensors(sd_f) if ni else None)
    last = "raw_fine" if ni else "raw_coarse"
    p = "fine" if ni else "coarse"
    keys = ("rgb_" + p, "depth_" + p, "acc_" + p, last)
    res32 = O.render_rays(rays, tc, tf, cfg, keep=keys)
    res64 = O.render_rays(rays, tc, tf, cfg, keep=keys, dtype=torch.float64)
    keep = res64[last][:, -1, 3].abs().numpy() > 1e-5
    pick = lambda res: {"rgb": res["rgb_" + p], "depth": res["depth_" + p], "acc": res["acc_" + p]}
    return pick(res32), pick(res64), keep


def scene_figures(cus, D, W, form, sampling):
    """What the host test's conditions are made of: rays left out, the std of the fp64 rgb, the spread of the fp64 depth, the
    mean acc."""
    _, ref64, keep = oracles(cus, D, W, form, sampling)
    return {"rays": int(keep.size), "left_out": int((~keep).sum()), "rgb_std": float(ref64["rgb"].std()),
            "depth_spread": float(ref64["depth"].max() - ref64["depth"].min()), "acc_mean": float(ref64["acc"].mean())}
