"""The legal network-shape domain of nwe_set_network / nwe_set_network_no_view_dirs / nwe_set_sampling: one table of named cases
shared by tests/test_shape_domain_oracle.py (CPU) and tests/test_gpu_shape_domain.py (GPU), like tests/input_domain.py is shared
by the input-domain tests.  Plain data plus builders; nothing here touches a GPU.

A case gives the coarse and the fine network (depth, width, skips; `output_ch` without view directions), the encoding widths
(num_freqs_3d / num_freqs_2d of the reference's YAML, handler.py:93-103: ONE embedding serves both networks), the form (view
directions or none), the sampling, and the seed and gains of the synthetic weights.  `build` returns the state dicts and the
first 37 rays of a 5 x 9 pinhole frame: three 16-ray workgroups of the fp32 kernel, the last one ragged.  The coarse network is
a thin fog (synthetic.thin_fog / thin_fog_output), so the inverse-CDF sampling is well conditioned; a case without importance
samples has no sampling to condition and keeps the plain random network, whose density has both signs.

Only NWE_PREC_F32 renders these shapes: every case is one the MFMA kernels have no instantiation for, either because a network's
shape is none of the six, or because the two networks differ (`mfma`: what Renderer.mfma_supported must say per network).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from nwe_amd import synthetic
from oracle import nerf_oracle as O

N_RAYS = 37                                      # 16 + 16 + 5
FRAME_H, FRAME_W = 5, 9
NEAR, FAR = 0.1, 10.0
F32, F64 = torch.float32, torch.float64

# include/nwe.h, nwe_set_network* / nwe_set_sampling
MAX_DEPTH, MAX_WIDTH = 16, 256
MAX_IN_XYZ, MAX_IN_DIR = 93, 63
MIN_OUTPUT_CH, MAX_OUTPUT_CH = 4, 256
MAX_SAMPLES, MAX_IMPORTANCE = 128, 256


@dataclass(frozen=True)
class Net:
    D: int
    W: int
    skips: Tuple[int, ...] = ()
    output_ch: int = 5                           # use_view_dirs=False only: rows of _output_linear (handler.py:110 passes 5)

    @property
    def skip(self) -> int:                       # the ABI's skip_layer
        return self.skips[0] if self.skips else -1


@dataclass(frozen=True)
class Case:
    name: str
    coarse: Net
    fine: Net
    freqs_xyz: int = 10
    freqs_dir: int = 4
    view_dirs: bool = True
    ns: int = 16
    ni: int = 24
    seed: int = 40
    w_gain: float = 2.0                          # gains of the FINE network (the last pass); the thin-fog coarse network keeps
    b_gain: float = 1.0                          # synthetic.make_state_dict's defaults
    white_background: bool = False
    feat_map: bool = False
    mfma: Tuple[bool, bool] = (False, False)     # Renderer.mfma_supported(0 / 1) as include/nwe.h states the six shapes

    @property
    def in_xyz(self) -> int:
        return O.embed_dim(self.freqs_xyz)

    @property
    def in_dir(self) -> int:
        return O.embed_dim(self.freqs_dir) if self.view_dirs else 0

    @property
    def last(self) -> Net:
        """The network of the last pass."""
        return self.fine if self.ni else self.coarse

    def shape(self, which: int) -> Tuple[int, int, int, int, int]:
        """What Renderer.set_network(which, ...) returns: (D, W, in_xyz, in_dir, skip_layer)."""
        n = self.fine if which else self.coarse
        return n.D, n.W, self.in_xyz, self.in_dir, n.skip

    def config(self) -> O.RenderConfig:
        return O.RenderConfig(n_samples=self.ns, n_importance=self.ni, freqs_xyz=self.freqs_xyz, freqs_dir=self.freqs_dir,
                              white_bkgd=self.white_background, endpoint_feat=self.feat_map)


def _same(D: int, W: int, skips: Tuple[int, ...] = (), **kw) -> Dict[str, Net]:
    return {"coarse": Net(D, W, skips), "fine": Net(D, W, skips), **kw}


# Seeds and gains: chosen on the fp64 oracle alone until the liveness conditions of tests/test_shape_domain_oracle.py hold (a
# 16 x 30 network with the default gain of 2 is dead: 0.67 of the variance survives each ReLU layer, acc = 0 on every ray).
CASES: List[Case] = [
    # depth 1: no hidden-to-hidden layer; W/2 = 1; in_xyz = in_dir = 3; the smallest sampling that has importance samples
    Case("1x2-freqs0-3+1", **_same(1, 2), freqs_xyz=0, freqs_dir=0, ns=3, ni=1, seed=40, w_gain=6.0, b_gain=2.0),
    # the skip at its lowest position; W/2 = 3
    Case("2x6-skip0-freqs1", **_same(2, 6, (0,)), freqs_xyz=1, freqs_dir=0, seed=48, w_gain=4.0),
    # kMaxDepth; a width that is no multiple of 4 or 16
    Case("16x30", **_same(16, 30), seed=56, w_gain=2.9),
    # the skip input enters the last trunk layer
    Case("6x64-skip4", **_same(6, 64, (4,)), seed=41),
    # the skip at D - 2, its highest position
    Case("7x32-skip5", **_same(7, 32, (5,))),
    # in_xyz = 93 and in_dir = 63: the bounds of the kernel's encoding rows; a width just under 256
    Case("3x254-skip1-freqs15", **_same(3, 254, (1,)), freqs_xyz=15, freqs_dir=10, ns=8, ni=12),
    # two MFMA shapes that together are f32-only: narrower coarse, wider fine
    Case("c4x128-f8x256", Net(4, 128), Net(8, 256, (4,)), mfma=(True, True)),
    # wider coarse, narrower fine: rows of the hidden buffers left from the coarse pass must not be read
    Case("c8x256-f2x16", Net(8, 256, (4,)), Net(2, 16), mfma=(True, False)),
    # neighbours of MFMA shapes
    Case("8x256-noskip", **_same(8, 256), ns=8, ni=12, seed=41),
    Case("8x256-skip3", **_same(8, 256, (3,)), ns=8, ni=12),
    Case("4x128-skip1", **_same(4, 128, (1,)), seed=42),
    Case("8x256-freqs9", **_same(8, 256, (4,)), freqs_xyz=9, ns=8, ni=12),
    # without view directions: _output_linear at both bounds of output_ch (channels 4.. are ignored)
    Case("novd-5x48-out4", Net(5, 48, (), 4), Net(5, 48, (), 4), view_dirs=False, seed=41),
    Case("novd-5x48-out256-freqs6", Net(5, 48, (), 256), Net(5, 48, (), 256), view_dirs=False, freqs_xyz=6),
    # two shapes in the 8-column ray form
    Case("novd-c4x128-f6x64", Net(4, 128), Net(6, 64, (4,)), view_dirs=False, mfma=(True, False)),
    # the largest S = 384 the ABI admits, and the smallest sampling
    Case("2x8-128+256", **_same(2, 8), freqs_xyz=4, freqs_dir=2, ns=128, ni=256, seed=40, w_gain=4.0),
    Case("2x8-2+0", **_same(2, 8), freqs_xyz=4, freqs_dir=2, ns=2, ni=0, seed=41, w_gain=4.0),
    Case("5x40-white", **_same(5, 40, (2,)), white_background=True, seed=42),
    # the endpoint feature at W/2 = 1, 3, 32 with a coarse network of another shape
    Case("feat-c2x8-f2x2", Net(2, 8), Net(2, 2), freqs_xyz=4, freqs_dir=2, feat_map=True, seed=55, w_gain=6.0, b_gain=2.0),
    Case("feat-c2x8-f3x6", Net(2, 8), Net(3, 6, (0,)), freqs_xyz=4, freqs_dir=2, feat_map=True, seed=40, w_gain=4.0),
    Case("feat-c3x32-f6x64", Net(3, 32), Net(6, 64, (4,)), feat_map=True, seed=41),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]

# the ragged-work test: the wider-coarse / narrower-fine case and the largest sampling
RAGGED_CASES = ("c8x256-f2x16", "2x8-128+256")
RAGGED_COUNTS = (1, 15, 16, 17, N_RAYS)


@dataclass
class Built:
    case: Case
    sd_c: Dict[str, np.ndarray]
    sd_f: Optional[Dict[str, np.ndarray]]        # None without importance samples
    rays: torch.Tensor                           # [37, 11 | 8]


def tensors(sd: Optional[Dict[str, np.ndarray]]) -> Optional[Dict[str, torch.Tensor]]:
    return None if sd is None else {k: torch.from_numpy(v) for k, v in sd.items()}


def frame_rays(use_view_dirs: bool = True, yaw_deg: float = -30.0) -> torch.Tensor:
    pose = O.camera_pose((0.0, -0.5, -0.76, 0.0, -90.0, 0.0), (0, 0, 0, yaw_deg, 0.0, 0.0))
    fx, fy, cx, cy = O.intrinsics(FRAME_H, FRAME_W)
    return O.create_rays(pose, FRAME_H, FRAME_W, fx, fy, cx, cy, NEAR, FAR, use_view_dirs)[0][:N_RAYS].contiguous()


def make_net(case: Case, net: Net, seed: int, w_gain: float = 2.0, b_gain: float = 1.0) -> Dict[str, np.ndarray]:
    return synthetic.make_state_dict(seed, net.D, net.W, in_xyz=case.in_xyz, in_dir=case.in_dir, skips=net.skips, w_gain=w_gain,
                                     b_gain=b_gain, use_view_dirs=case.view_dirs, output_ch=net.output_ch)


def build(case: Case) -> Built:
    fog = synthetic.thin_fog if case.view_dirs else synthetic.thin_fog_output
    if case.ni:
        sd_c = fog(make_net(case, case.coarse, case.seed))
        sd_f = make_net(case, case.fine, case.seed + 1, case.w_gain, case.b_gain)
    else:
        sd_c, sd_f = make_net(case, case.coarse, case.seed + 1, case.w_gain, case.b_gain), None
    return Built(case, sd_c, sd_f, frame_rays(case.view_dirs))


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(built case, fp32 oracle outputs, fp64 oracle outputs): computed once per case and shared; nobody writes to it."""
    b = build(BY_NAME[name])
    cfg = b.case.config()
    res32 = O.render_rays(b.rays, tensors(b.sd_c), tensors(b.sd_f), cfg)
    res64 = O.render_rays(b.rays, tensors(b.sd_c), tensors(b.sd_f), cfg, dtype=F64)
    return b, res32, res64


def last_pass(res: Dict[str, torch.Tensor], case: Case) -> Tuple[torch.Tensor, torch.Tensor]:
    """(acc [R], raw [R, S, 4]) of the last pass of oracle outputs."""
    p = "fine" if case.ni else "coarse"
    return res["acc_" + p], res["raw_" + p][..., :4]


def forward_weight_elements(sd: Dict[str, np.ndarray]) -> int:
    """Weight elements the forward pass of nerf_model.py:45-83 multiplies by: the trunk and the four heads, or, without view
    directions, the trunk and every row of _output_linear (the module's _views_linears.0 is then never called)."""
    used = [k for k in sd if k.endswith(".weight") and k.startswith("_pts_linears.")]
    used += ["_output_linear.weight"] if "_output_linear.weight" in sd else \
        ["_views_linears.0.weight", "_feature_linear.weight", "_alpha_linear.weight", "_rgb_linear.weight"]
    return int(sum(sd[k].size for k in used))
